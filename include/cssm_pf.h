/*
 * cssm_pf.h -- C ABI of libcssm_pf, the MI355X (gfx950) bootstrap particle filter.
 *
 * The reference (jonnylaw/ComposableStateSpaceModels, Scala/JVM) has no FFI; this header is
 * the FFI its `ParticleFilter` seam would bind.  Every entry point
 * cites the reference symbol it replaces as  model/<File>.scala:<lines>  (paths relative to
 * src/main/scala/com/github/jonnylaw/ of the reference).  The JNI/Scala binding a maintainer
 * would add is shown in INTEGRATION.md and shipped as source under jvm/.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, all floating point is IEEE fp64.
 *   - Return value 0 (CSSM_OK) or a negative CSSM_E* code; cssm_last_error() returns a
 *     thread-local message for the last failing call on this thread.  The reference throws
 *     from inside stepFilter (model/Sde.scala:214, model/Model.scala:150); the JNI glue turns
 *     a non-zero code into a RuntimeException.
 *   - The handle owns all device memory and its HIP stream; the caller owns every
 *     host buffer passed in or out.  Pointers documented as "host" must be host memory,
 *     pointers documented as "device" must be device memory of the handle's GPU.
 *   - A handle is not re-entrant; distinct handles share nothing mutable and may be driven
 *     from different threads (two PMMH chains: examples/DetermineParameters.scala:68-69).
 *     Every entry point selects the handle's device itself, so calls may arrive on any thread
 *     (Akka dispatcher threads: model/ParticleFilter.scala:163-166).
 *   - Random numbers and reductions follow include/cssm_numerics.h (the numerics contract).
 *   - Stated fp64 tolerance to the reference's literal arithmetic (sequential fp64 sums and cumulative weights, platform
 *     libm, rescaling by the max -- model/ParticleFilter.scala:124-128, model/Resampling.scala:21-24,57) under the same
 *     variates:  |ll - ll_literal| <= 1e-9 * T  for a series of T observations (measured: 1e-13), and at most a fraction
 *     1e-4 of the ancestor indices of the first weighted observation differ (measured: none).  The reference's TreeMap
 *     keeps the LAST particle of equal cumulative weights (:57); the library keeps the first, which owns the mass
 *     (deviation D3): with that quirk switched on in the oracle, 0.4 % of the slots at N = 2^16 go to a
 *     particle of negligible weight instead, after which the two runs agree as two realisations of one estimator do.
 *     Against the CPU restatement that shares the contract (oracle/), everything is bit-identical.
 *     tests/test_gpu_parity.py asserts all of it on the GPU.
 */
#ifndef CSSM_PF_H
#define CSSM_PF_H

#if !defined(__HIPCC_RTC__)
#include <stddef.h>
#include <stdint.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---------------------------------------------------------------------- */
#define CSSM_OK 0
#define CSSM_EINVAL_DESC (-1) /* malformed model descriptor (reference: Failure(...) at model/Model.scala:44-47) */
#define CSSM_EHIP (-2)        /* a HIP runtime call failed / no gfx950 device */
#define CSSM_ESHARD (-3)      /* inconsistent sharding arguments */
#define CSSM_ENOMEM (-4)
#define CSSM_ENONFINITE (-5)  /* NaN log-weight or all weights zero (reference: breeze `require` throws) */
#define CSSM_EINVAL_ARG (-6)
#define CSSM_ESTATE (-7)      /* call out of sequence (e.g. step before init) */
#define CSSM_ERCCL (-8)       /* librccl.so could not be loaded, or an RCCL call failed */

/* ---- model descriptor ------------------------------------------------------------------- */
/* Latent SDE of one leaf: model/Sde.scala:98-124 (Brownian), :69-96 (GenBrownian),
 * :129-163 (OU), :23-43 (trait default Euler-Maruyama, here with affine drift a + b*x and
 * constant diagonal diffusion g). */
#define CSSM_SDE_BROWNIAN 0
#define CSSM_SDE_GEN_BROWNIAN 1
#define CSSM_SDE_OU 2
#define CSSM_SDE_EULER_AFFINE 3

/* Linear map f of one leaf: "first component" model/Model.scala:271 (also :153,184,250,296,
 * 328,347,366) or seasonal model/Model.scala:217-225. */
#define CSSM_F_FIRST 0
#define CSSM_F_SEASONAL 1

/* Observation model of the LEFTMOST leaf (model/Model.scala:118-132):
 * Poisson model/Model.scala:266-274; Gaussian (LinearModel :241-259, SeasonalModel :227-233);
 * LGCP model/Model.scala:363-369 with the FilterLgcp step model/ParticleFilter.scala:169-227. */
#define CSSM_OBS_POISSON 0
#define CSSM_OBS_GAUSSIAN 1
#define CSSM_OBS_LGCP 2
/* "next" rows of SURVEY.md 8f-1, all with f = first component of the leftmost leaf: */
#define CSSM_OBS_NEGBIN 3     /* NegativeBinomialModel  model/Model.scala:168-196, size = exp(scale)          */
#define CSSM_OBS_ZIP 4        /* ZeroInflatedPoisson    model/Model.scala:281-309, p = logistic(scale)        */
#define CSSM_OBS_BERNOULLI 5  /* BernoulliModel         model/Model.scala:315-337 (+-6 clamp, -1e99 floor)    */
#define CSSM_OBS_STUDENT_T 6  /* StudentsTModel         model/Model.scala:144-161, v = exp(scale), obs_df     */
#define CSSM_OBS_BETA 7       /* BetaModel              model/Model.scala:339-353, Beta(exp(-gamma), 1)       */

#define CSSM_MAX_DIM 16     /* total latent dimension d (sum over leaves) */
#define CSSM_MAX_LEAVES 16

/*
 * One leaf of the composed model, left-to-right in Tree.flatten order (model/Tree.scala:49-53).
 * Parameter arrays hold the STORED (unconstrained) values exactly as ParamNode/SdeParameter
 * hold them (model/SdeParameters.scala:176-205) -- log c0, log sigma, and for OU the value
 * the reference later passes through `logistic` (model/Sde.scala:136).  The library applies
 * exp/logistic itself (cssm_exp) and repeats each array cyclically to `dim`
 * (Sde.buildParamRepeat, model/Sde.scala:177-179).  For CSSM_SDE_EULER_AFFINE mu = a,
 * phi = b, sigma = g are taken as they are (a user-defined Sde has no stored transform);
 * c0 is still a log-variance.
 */
typedef struct cssm_leaf_desc {
  int32_t sde_kind;
  int32_t dim;
  int32_t f_kind;
  int32_t period;     /* CSSM_F_SEASONAL: model/Model.scala:205 */
  int32_t harmonics;  /* CSSM_F_SEASONAL: dim must equal 2*harmonics */
  int32_t has_scale;  /* ParamNode.scale is Some(_) (model/Parameters.scala:14) */
  double scale;       /* stored scale; Gaussian uses sd = exp(scale) (model/Model.scala:244) */
  int32_t n_m0, n_c0, n_mu, n_phi, n_sigma;
  int32_t reserved;
  const double* m0;
  const double* c0;
  const double* mu;    /* GenBrownian, OU, EulerAffine(a) */
  const double* phi;   /* OU, EulerAffine(b) */
  const double* sigma; /* all kinds */
} cssm_leaf_desc;

typedef struct cssm_model_desc {
  int32_t n_leaves;
  int32_t obs_kind;
  int32_t lgcp_precision; /* FilterLgcp.precision (model/ParticleFilter.scala:172) */
  int32_t obs_df;         /* CSSM_OBS_STUDENT_T: degrees of freedom (`df: Int`, model/Model.scala:144) */
  const cssm_leaf_desc* leaves;
} cssm_model_desc;

typedef struct cssm_pf cssm_pf; /* opaque handle */

/* ---- lifetime ---------------------------------------------------------------------------- */

/* Build a filter for `n_particles` particles on HIP device `device`.  Replaces the
 * construction `Filter(mod, resample)` / `FilterLgcp(mod, resample, precision)`
 * (model/ParticleFilter.scala:233-235, :169-172) with resample = systematicResampling. */
int cssm_pf_create(const cssm_model_desc* desc, uint64_t n_particles, uint64_t seed, int device,
                   cssm_pf** out);

/* Same, for one shard of a filter whose N_global particles are split over `world` GPUs (one
 * process per GPU).  This rank owns global particles and resampling slots
 * [first, first + n_local).  Random variates are keyed by GLOBAL particle id, so results do
 * not depend on `world`.  The collectives between the stages are the caller's (torch.distributed
 * over RCCL): see the cssm_pf_shard_* stage calls below. */
int cssm_pf_create_shard(const cssm_model_desc* desc, uint64_t n_global, uint64_t first,
                         uint64_t n_local, uint64_t seed, int device, void* hip_stream,
                         cssm_pf** out);

void cssm_pf_destroy(cssm_pf* pf);

/* New parameters for the same model structure, without reallocating: one call per PMMH
 * proposal (model/PMMH.scala:71, `pf(propParams)`).  Allowed at any moment, also between the observations of a running series
 * (the cloud stays, the next transition and weights use the new parameters).  A descriptor of another structure is refused with
 * CSSM_EINVAL_DESC and leaves the handle exactly as it was. */
int cssm_pf_set_params(cssm_pf* pf, const cssm_model_desc* desc);

/* New Philox key (a fresh filter run must not reuse variates). */
int cssm_pf_reseed(cssm_pf* pf, uint64_t seed);
/* The key a driver should hand to cssm_pf_reseed for its `run`-th filter run under one user seed: a PRF of (seed, run)
 * (include/cssm_numerics.h, cssm_derive_key), never seed + run -- chains seeded s and s + 1 would otherwise replay each
 * other's filter randomness one iteration apart.  cssm_pmmh_run uses run = iteration + 1. */
uint64_t cssm_pf_run_key(uint64_t seed, uint64_t run);

/* ---- streaming mode: one native call per observation -------------------------------------- */

/* initialiseState (model/ParticleFilter.scala:105-108): N draws m0 + sqrt(c0) z; ll = 0,
 * ess = N, t = t0, step counter = 0. */
int cssm_pf_init(cssm_pf* pf, double t0);

/* FilterInit.initialiseState (model/ParticleFilter.scala:257-260): replicate one state
 * (host pointer, d doubles in flatten order) N times. */
int cssm_pf_init_from(cssm_pf* pf, double t0, const double* state_d);

/* stepFilter (model/ParticleFilter.scala:116-132; LGCP: :210-226).  `has_obs` = 0 is the
 * `None` branch (:121): propagate only, ll and ess unchanged.  ll_out = accumulated
 * log-likelihood, ess_out = floor(1 / sum(normalised w^2)) (:431-434).
 * t is not compared with the handle's clock on the host: a time BEFORE it gives a negative increment, the transition's variance
 * and with it every log-weight is NaN, and a weighted step returns CSSM_ENONFINITE like any other step whose weights are unusable
 * (LGCP: the number of sub-steps is ceil(dt / delta), so a negative increment is the caller's error and undefined).  After a call
 * that returned CSSM_ENONFINITE the series is over: the cloud is undefined until cssm_pf_init / _init_from / a batch call draws a
 * new one, which then behaves exactly as on a new handle. */
int cssm_pf_step(cssm_pf* pf, double t, double obs, int has_obs, double* ll_out, int32_t* ess_out);

/* stepFilter split at the resampler, for a `Resample[A]` the library does not have natively (any host function:
 * model/package.scala:23; Resampling.indentity, model/Resampling.scala:29).  cssm_pf_propagate does :117-124 (propagate the
 * cloud to t, weigh it; `has_obs` = 0: propagate only); the host reads the proposed cloud and the log-weights
 * (cssm_pf_get_proposed, cssm_pf_get_logw), forms w1 = exp(w - max), applies its resampler, and hands the resampled cloud
 * (SoA, d x N, host) back with cssm_pf_adopt together with the new ll and ess (:126-130).  A parity path: the cloud crosses
 * PCIe twice per observation.  After cssm_pf_propagate without cssm_pf_adopt the proposed cloud is the current one.
 * Between the two calls parameters, key and options may change and every read-only call may run.  No native resampling stands
 * behind a propagated or adopted cloud: cssm_pf_get_ancestors gives the identity, and after cssm_pf_adopt cssm_pf_get_proposed
 * gives the adopted cloud (it replaced the proposed one in place).  A weighted cssm_pf_propagate keeps log-weights
 * (cssm_pf_get_logw); one WITHOUT a datum stores none and leaves weights / log-weights and their getters as the last weighted
 * step left them. */
int cssm_pf_propagate(cssm_pf* pf, double t, double obs, int has_obs);
int cssm_pf_adopt(cssm_pf* pf, const double* state_dN, double ll, int32_t ess);

/* ---- batch mode: one native call for all T observations ----------------------------------- */

/* llFilter (model/ParticleFilter.scala:137-140): t0 = min t, init, fold stepFilter over the
 * data in the order given.  Optional outputs (may be NULL): ll_t[T] running log-likelihood
 * after each datum, ess_t[T].  No host synchronisation happens inside the loop.
 * T = 0 is refused with CSSM_EINVAL_ARG (the reference's minBy throws on an empty Vector) by all three batch calls and leaves the
 * handle as it was; an observation without a datum reports the ESS before it (a continued call that starts on one: the ESS the
 * handle had -- N behind a new cloud, the caller's behind cssm_pf_adopt). */
int cssm_pf_ll_filter(cssm_pf* pf, const double* t, const double* y, const uint8_t* has_obs,
                      size_t T, double* ll_out, double* ll_t, int32_t* ess_t);
/* The same for T MORE observations of a filter that is already running (initialised by cssm_pf_init / _init_from, or left
 * behind by a batch run or by streaming steps): no initial cloud is drawn, the first time increment is taken from the
 * handle's clock, and observation s of this call is observation (steps so far + s) of the filter -- what Flow.scan(init)
 * (stepFilter) does with the next T elements of the stream (model/ParticleFilter.scala:163-166), without a host round trip
 * per element.  *ll_out = the log-likelihood accumulated since the filter was initialised; ll_t / ess_t: this call's
 * observations.  cssm_pf_ll_filter(t[0..a)) followed by cssm_pf_ll_filter_more(t[a..T)) leaves the same bits as
 * cssm_pf_ll_filter(t[0..T)). */
int cssm_pf_ll_filter_more(cssm_pf* pf, const double* t, const double* y, const uint8_t* has_obs, size_t T,
                           double* ll_out, double* ll_t, int32_t* ess_t);

/* filter (model/ParticleFilter.scala:152-158): as llFilter, and path[(T+1)*d] receives one
 * uniformly picked particle of the initial cloud and of the cloud after every datum
 * (Resampling.sampleOne, model/Resampling.scala:151-154), row s = time index, d doubles. */
int cssm_pf_filter(cssm_pf* pf, const double* t, const double* y, const uint8_t* has_obs, size_t T,
                   double* ll_out, double* ll_t, int32_t* ess_t, double* path);

/* Device time of the last cssm_pf_ll_filter / cssm_pf_filter loop (HIP events on the
 * handle's stream around the T steps, init excluded), in milliseconds.  The events are recorded only
 * with CSSM_OPT_LOOP_EVENTS = 1 (below; environment CSSM_LOOP_EVENTS=1 sets that default): CSSM_ESTATE otherwise. */
int cssm_pf_last_loop_ms(cssm_pf* pf, float* ms_out);

/* Device time of the last batch call (cssm_pf_ll_filter_more, a sharded cssm_pf_shard_continue + series + status) WITHOUT event packets:
 * the kernel that brings the call's first record stamps the GPU's constant 100 MHz clock (s_memrealtime) at its first instruction, the
 * call's closing kernel (k_finish) stamps it again and hands both to the host with the results.  *us_out = first instruction of the
 * call's first kernel -> the closing kernel's copy of the results, in microseconds (resolution 10 ns).  What bench.py reports per
 * timed leg (`device_ms_each`) beside the host's wall time.  CSSM_ESTATE if the last call left no pair of stamps (a call that drew
 * a new cloud: the scalars are reset behind its first kernel; a call whose records travelled by hipMemcpyAsync -- environment
 * CSSM_UPLOAD_MEMCPY=1 -- where no kernel carries record 0: the stamp is then cleared, never left over from an earlier call).
 * The interval never spans more than the one call. */
int cssm_pf_last_device_us(cssm_pf* pf, double* us_out);

/* 1 if nothing is queued or running on the handle's stream (hipStreamQuery: every launch of the calls so far has completed as the runtime
 * sees it), 0 if work is still pending, negative on a HIP error.  The batch drivers return on their closing kernel's completion word;
 * a caller that wants the runtime's own confirmation (bench.py does, right behind its timed region) asks here -- no wait, no packet. */
int cssm_pf_stream_idle(cssm_pf* pf);

/* Debug/verification options.  cssm_pf_set_option may be called at ANY moment, also between two observations of a running series and
 * between cssm_pf_propagate and cssm_pf_adopt: a new value holds from the next launch on, whatever the filter left behind.  Every
 * option below except CSSM_OPT_RESAMPLER is a VERIFICATION SWITCH: results are bit-identical in every setting and across every
 * switch in the middle of a series (tests/test_gpu_call_sequences.py drives reused handles through seeded sequences of switches and
 * compares every call with the oracle).  CSSM_OPT_RESAMPLER changes results: from the next weighted observation on the new
 * resampler selects the ancestors.  An unknown option or a value outside an option's range where one is checked (CSSM_OPT_RESAMPLER,
 * a negative CSSM_OPT_FORECAST_CAP) is refused with CSSM_EINVAL_ARG and changes nothing.
 * CSSM_OPT_EXACT_OFFSPRING = 1 makes the offspring kernel evaluate the
 * contract's exact predicate for every particle instead of only where its fp64 position estimate is
 * within the error band of a slot boundary; results are identical by construction (tests compare).
 * Value 2 (systematic resampling): every third particle only -- threads then hand over single particles, as the
 * fast path does when one of them is close to a boundary. */
#define CSSM_OPT_EXACT_OFFSPRING 1
/* CSSM_OPT_RESAMPLER selects the `Resample[A]` the filter was constructed with (model/ParticleFilter.scala:
 * 233-235): systematic (model/Resampling.scala:63-72, default), stratified (:78-86) or multinomial (:92-96).
 * The reference's residualResampling (:130-146) indexes `Vector.range(1, m)` with draws from [0, n) and cannot
 * run as written; it is not offered.  Sharded handles support systematic and stratified resampling (the grid points of both are
 * keyed by GLOBAL slot and ordered, so the ancestors of a rank's slots are its own particles plus its neighbours' boundary blocks);
 * a multinomial resampler draws every slot's ancestor from the whole cloud and stays single-GPU. */
#define CSSM_OPT_RESAMPLER 2
#define CSSM_RESAMPLE_SYSTEMATIC 0
#define CSSM_RESAMPLE_STRATIFIED 1
#define CSSM_RESAMPLE_MULTINOMIAL 2
/* CSSM_OPT_FUSED_SUMS (default 1; a verification switch like CSSM_OPT_WHOLE_TILES -- results are identical, both settings apply
 * cssm_ref_choose): k_propagate also forms the fixed-point sums of exp(w - c) (c = the observation's reference level,
 * cssm_numerics.h) -- the log-sum-exp normalisation inside the fused kernel: 2 kernels per observation.  When the max rules c
 * out (an outlying observation) the batch drivers put the series on hold at that observation, redo its sums relative to the
 * max and carry on; streaming cssm_pf_step does the same within the call.  0 = the sums are always a pass of their own after
 * the max is known (k_tile_sums, 3 kernels per observation) -- the path LGCP, the multinomial resampler and a redone observation
 * run anyway; measured slower at every size (20.0 vs 18.7 us at N = 100 000, 35.4 vs 34.0 at 2^20, 356 vs 336 at 2^24). */
#define CSSM_OPT_FUSED_SUMS 3
/* CSSM_OPT_WHOLE_TILES (default 0): a verification switch over the launch geometry of the propagate kernel (results are
 * bit-identical in every setting).  Automatic (0): clouds below 2^20 particles run ONE tile of the kernel per block (512
 * particles for d <= 8, 256 for d >= 9: the single-tile kernel requests everything position-dependent in its first round of
 * loads and draws the normals while the gathered rows travel; k_offspring totals one pair of sums per block); from 2^20 on a
 * block owns a whole unit of 1024 * k particles and runs (1) the same kernel tile after tile while a unit has at most 8
 * tiles, else (2) the software-pipelined kernel (d <= 3) or (3) one tile per block again with k_reduce_units folding the
 * blocks' sums into <= 1024 unit sums (d >= 4).  1 / 2 / 3 force that geometry at every size: the kernels of the large
 * clouds can then be checked against the oracle at sizes the oracle finishes in seconds.
 * (Options 4 and 5 of rounds 1-2 -- a persistent one-launch-per-series kernel and a one-launch-per-observation kernel, both
 * bit-identical and both measured slower than two launches per observation -- were removed in round 3; docs/history/LABNOTES_rounds1-3.md (sections 5b-5c) keeps
 * the record, git history the code.) */
#define CSSM_OPT_WHOLE_TILES 6
/* CSSM_OPT_GROUP_SUMS (default 1; a verification switch: results are bit-identical either way).  Where k_propagate runs one
 * fused-sums block per unit of a single-GPU cloud (every cloud of 2^20 particles or more that is not on geometry 3; smaller ones
 * under CSSM_OPT_WHOLE_TILES = 1 or 2 from 64 units on) its blocks also add their unit sums, limb by limb, to the sums of groups
 * of 32 units, and k_offspring's blocks read 32 group sums + the 32 unit sums of their own group instead of all 1024 unit sums
 * (16 KiB per block through the L2s).  0 = every block totals every unit sum, as before. */
#define CSSM_OPT_GROUP_SUMS 7
/* CSSM_OPT_SPECIALISE (default 1; results are bit-identical either way): the fused kernel holds the model's STRUCTURE -- per latent
 * component its SDE, its place in the f map, where its leaf ends -- and its observation model at compile time, as the reference's
 * models are composed at compile time (model/Model.scala:110-136): ahead-of-time instantiations for BASELINE's configurations, and for
 * every other model (d <= 12) one compiled at RUN TIME with hipRTC from the library's own kernel sources (~1 s per kernel the first time
 * a structure is seen; kept on disk afterwards: $CSSM_RTC_CACHE, else rtc_cache/ next to the library).  If the runtime compiler is
 * unavailable one line on stderr says so and the structure-as-data kernel runs; environment CSSM_RTC=0 does the same on purpose.
 * 0: always the structure-as-data kernel (bench.py reports its roofline fraction beside the specialised kernel's); 2 (verification):
 * the run-time-compiled kernel also where an ahead-of-time instantiation exists (tests compare the two). */
#define CSSM_OPT_SPECIALISE 8
/* CSSM_OPT_LOOP_EVENTS (default 0): the batch drivers record a HIP event before the first and behind the last per-observation kernel of a
 * call, which cssm_pf_last_loop_ms then reads.  Off by default: the two event packets cost a 20-observation call about 5 us (the one
 * between the last kernel and the call's closing kernel holds the queue for ~4 us). */
#define CSSM_OPT_LOOP_EVENTS 9
/* CSSM_OPT_WAVE_SUMS (default 1; a verification switch: results are bit-identical either way).  Single GPU, systematic resampling, clouds of
 * 2^20 particles and more on the tile-after-tile launch: every wave of the fused kernel owns a contiguous quarter of its block's unit and
 * stores the exact fixed-point sum of its weights; the resampling kernel (k_offspring_wave) takes a wave's prefix from those sums and the
 * group sums and runs the rest of its prefix arithmetic in fp64 -- no conversion to the 2^-96 grid and no 128-bit scan per weight, one block
 * barrier per block; the contract's exact predicate where the fp64 estimate is within its error band of a slot boundary, as before.
 * The mapping costs the fused kernel 1-4 % at d <= 2 and up to 10 % at d = 3 on the fastest boxes (a block streams four ranges per row
 * instead of one), the resampling kernel gains 14-16 % from 2^21 particles on and nothing at 2^20 (one tile per unit): 1 applies it to clouds
 * whose units have several tiles (more than 2^20 particles) of models with at most two latent components -- where the STEP gains --, 2
 * (verification, A/B) wherever the geometry allows, 0 = never: k_offspring_self (every weight converted and scanned in 128 bits). */
#define CSSM_OPT_WAVE_SUMS 10
/* CSSM_OPT_FORECAST_CAP (value in KiB; default 0 = 1 GiB): cssm_pf_forecast runs its horizons in chunks whose order keys
 * ((d + 2) x N x 8 bytes per horizon) fit in this many KiB (at least one horizon per chunk).  Results do not depend on it (tests
 * lower it to run the chunked path at small N). */
#define CSSM_OPT_FORECAST_CAP 11
/* CSSM_OPT_FLEET_SELECT (fleets only; default 0): how cssm_fleet_forecast takes the two order statistics of a row inside the series'
 * workgroup -- 0: chosen by N (today: the sort at every N), 1: a bitonic sort of the row's keys in LDS, 2: a radix select over them in LDS.  Both are exact: the
 * results do not depend on it (tests/test_gpu_fleet_forecast.py); it exists for measurements. */
#define CSSM_OPT_FLEET_SELECT 12
/* CSSM_OPT_INTERP_CAP (fleets only, cssm_fleet_set_option; value in KiB; default 0 = 1 GiB, negative refused): cssm_fleet_interpolate runs the
 * fleet in chunks of series whose lineage history ((T_k + 1) x N x (8 d + 4) bytes per series) fits in this many KiB -- one series at
 * least per chunk, never a part of one.  Results do not depend on it (tests lower it to run the chunked path on a small fleet). */
#define CSSM_OPT_INTERP_CAP 13
/* CSSM_OPT_SMOOTH_STAGING (fleets only, cssm_fleet_set_option; default 0): where cssm_fleet_smooth's backward simulation reads the gathered
 * cloud of a time index from -- 0: the block's LDS where d x N x 8 bytes fit, else the slice through L2; 1: never LDS.  The results do not
 * depend on it (tests/test_gpu_fleet_smooth.py); it exists for tests and measurements. */
#define CSSM_OPT_SMOOTH_STAGING 14
/* CSSM_OPT_SMOOTH_TILE (single handles only, cssm_pf_set_option; default 0 = CSSM_SMOOTH_TILE): the slots a block of cssm_pf_smooth's
 * backward kernels stages in LDS -- a multiple of 64, at least 64; anything else is CSSM_EINVAL_ARG and changes nothing.  The results do
 * not depend on it (tests/test_gpu_smooth.py lowers it to put many tiles under a small cloud). */
#define CSSM_OPT_SMOOTH_TILE 15
#define CSSM_SMOOTH_TILE 512
int cssm_pf_set_option(cssm_pf* pf, int option, int value);
/* Counters of the run-time specialisation in this process: out4 = {kernels compiled, kernels loaded from the disk cache, launches of
 * run-time-compiled kernels, failures (each reported once on stderr)}. */
int cssm_rtc_info(uint64_t* out4);

/* Per-kernel device time, measured with HIP events recorded on the handle's stream directly
 * before and after every kernel launch of the batch loop (bench.py's `roofline` figure).
 * Enabling it inserts event records between kernels, so whole-loop throughput is measured with
 * profiling OFF.  The event packets themselves take time on the queue (about 2 us per bracketed launch on MI355X): the
 * caller can calibrate that in place as (loop time with profiling - loop time without) / bracketed launches, both loop
 * times from cssm_pf_last_loop_ms (bench.py does, and its figure then agrees with rocprofv3's kernel trace). */
#define CSSM_K_PROPAGATE 0   /* fused gather + propagate + weight + block max (+ fixed-point sums with CSSM_OPT_FUSED_SUMS) */
#define CSSM_K_TILE_SUMS 1   /* exp(w - level), fixed-point unit sums */
#define CSSM_K_OFFSPRING 2   /* unit prefix, ll / ess, cumulative weights -> end slots -> ancestor indices */
#define CSSM_K_REDUCE 3      /* k_reduce_units: the sums of k_propagate's single-tile blocks -> unit sums (large clouds) */
#define CSSM_K_PACK 4        /* sharded: k_boundary_pack (segment headers + boundary rows of the single-collective exchange) */
#define CSSM_K_EXPAND 5      /* sharded: k_offspring_expand_spec (offspring of the own particles + expansion of the received rows) */
#define CSSM_K_COLLECTIVE 6  /* sharded, collectives issued by the library: the RCCL kernel(s) of one observation's exchange */
#define CSSM_PROFILE_NKERNELS 7
int cssm_pf_profile(cssm_pf* pf, int enable);
int cssm_pf_profile_read(cssm_pf* pf, double* total_ms, uint64_t* launches);
/* ---- diagnostics of the numerics contract --------------------------------------------------- */

/* Evaluates one function of include/cssm_numerics.h ON THE DEVICE for n arguments (so that a caller holding the host
 * build of the same header can check that both builds agree bit for bit; the parity tests do).
 *   CSSM_FN_EXP / CSSM_FN_LOG / CSSM_FN_LOG_UNIT: out[i] = f(x[i])
 *   CSSM_FN_SINCOS2PI: out[2i] = sin, out[2i+1] = cos of 2 pi x[i]
 *   CSSM_FN_FIX: out holds 2 n 64-bit words (lo, hi) of cssm_fix_from_double(x[i]), written as raw bits
 *   CSSM_FN_PAIRED_NORMALS: x = {seed, first global particle id, step, tag, d} as doubles (n = 5 is ignored: n_out
 *                           particles are drawn); out[i * d + k] = normal k of particle first + i
 * n_out = number of doubles `out` can hold. */
#define CSSM_FN_EXP 0
#define CSSM_FN_LOG 1
#define CSSM_FN_LOG_UNIT 2
#define CSSM_FN_SINCOS2PI 3
#define CSSM_FN_FIX 4
#define CSSM_FN_PAIRED_NORMALS 5
#define CSSM_FN_SINCOS_U24 6   /* out[2i] = sin, out[2i+1] = cos of 2 pi k / 2^24, k = (uint32_t)x[i] < 2^24 (cssm_sincos_u24) */
#define CSSM_FN_SQRT_RADIUS 7  /* out[i] = cssm_sqrt_radius(x[i]), x[i] = +-0 or in [2^-39, 55.5] */
#define CSSM_FN_EXP_LE0 8      /* out[i] = cssm_exp_le0(x[i]), x[i] <= 2^-20 and not NaN (-inf allowed) */
#define CSSM_FN_LGAMMA 9       /* out[i] = cssm_lgamma(x[i]): the samplers and the IF2 kernel evaluate it per lane */
#define CSSM_FN_LGAMMA_KP1 10  /* out[i] = cssm_lgamma_kp1((long long)x[i]), x[i] an integer in [0, 2^62] */
int cssm_contract_eval(int device, int fn, const double* x, size_t n, double* out, size_t n_out);

/* On-box streaming ceiling: GB/s (read + write) of a plain 16-bytes-per-lane device-to-device copy of `bytes` bytes,
 * HIP-event timed over `reps` launches.  bench.py reports k_propagate's rate against it beside the 8 TB/s specification
 * ("measure an on-box copy ceiling too and report both fractions"). */
int cssm_diag_copy_ceiling(int device, size_t bytes, int reps, double* gbps_out);

/* ---- inspection (parity tests, `PfState.particles` on demand) ------------------------------ */

uint64_t cssm_pf_num_particles(const cssm_pf* pf); /* local particle count */
int32_t cssm_pf_dim(const cssm_pf* pf);            /* total latent dimension d */

/* Current cloud, i.e. the RESAMPLED particles of the last step (PfState.particles,
 * model/ParticleFilter.scala:35), SoA: out[k*N + i] = component k of particle i.  Host ptr. */
int cssm_pf_get_particles(cssm_pf* pf, double* out_dN);
/* Ancestor indices of the last resampling (slot i <- particle anc[i]); host pointer, N. */
int cssm_pf_get_ancestors(cssm_pf* pf, uint32_t* out_N);
/* Log-weights of the last weighted step, before resampling (model/ParticleFilter.scala:123) -- where the handle keeps them: LGCP
 * filters, the multinomial resampler, cssm_pf_propagate, CSSM_OPT_FUSED_SUMS = 0, an observation that was redone relative to
 * the max.  Otherwise CSSM_ESTATE: the fused kernel stores the WEIGHTS in their place, see cssm_pf_get_weights.  Which of the two is
 * kept follows the LAST weighted observation (not the options' current values); exactly one of the two getters answers.  Before the
 * first weighted observation since the cloud was drawn the buffer's contents are unspecified. */
int cssm_pf_get_logw(cssm_pf* pf, double* out_N);
/* The weights w1_i = exp(min(w_i - c, 2^-20)) of the last weighted step -- what stepFilter hands its resampler as the second
 * argument, rescaled by the observation's reference level c instead of the max (model/ParticleFilter.scala:125-126;
 * include/cssm_numerics.h, "reference level") -- and *level_out = c (may be NULL).  CSSM_ESTATE where log-weights are kept. */
int cssm_pf_get_weights(cssm_pf* pf, double* out_N, double* level_out);
/* Propagated, not yet resampled particles of the last step (x1 at :118), SoA, host pointer. */
int cssm_pf_get_proposed(cssm_pf* pf, double* out_dN);

/* getIntervals (model/ParticleFilter.scala:415-424) of the current cloud, computed on the device so that
 * the streaming consumer (examples/Filtering.scala:29) never copies N particles back: per latent
 * component the mean (meanState, :465-479) and the two order statistics of getCredibleInterval
 * (:488-502: sorted(N - index - 1), sorted(index - 1), index = floor(interval*N)); for
 * eta = link(f(x, t)) the order statistics of getOrderStatistic (:455-460: sorted(N - index),
 * sorted(index)) and eta_of_mean = link(f(stateMean, t)) (:420).  Host pointers, d doubles each for the
 * state outputs; any may be NULL.  Order statistics are exact (radix selection); the means are plain
 * fp64 sums (agreement with the reference's sequential sum: ~1e-13 relative). */
int cssm_pf_summary(cssm_pf* pf, double interval, double* state_mean, double* state_lower, double* state_upper,
                    double* eta_of_mean, double* eta_lower, double* eta_upper);

/* Filtered intervals of every observation in ONE call: `filter`, then getIntervals of every emitted state
 * (examples/Filtering.scala:23-32) -- cssm_pf_ll_filter with a cssm_pf_summary row behind the initial cloud and behind every record,
 * enqueued between the observations' launches with no host round trip and one synchronisation per call.
 *   row 0      the initial cloud, at t0 = min t
 *   row s + 1  the resampled cloud behind record s (a record without a datum: the moved cloud through identity ancestors)
 * state_mean / state_lower / state_upper: [T + 1][d]; eta_of_mean / eta_lower / eta_upper: [T + 1]; any output may be NULL.  Every row
 * has the BITS cssm_pf_summary(pf, interval, ...) gives at that moment of the loop cssm_pf_init; summary; (cssm_pf_step; summary) x T;
 * ll_out, ll_t, ess_t and the handle (cloud, ancestors, clock, observation index, LGCP level) are cssm_pf_ll_filter's.  Served: every
 * handle cssm_pf_ll_filter serves (every observation model, the LGCP, the three native resamplers); a sharded handle is CSSM_ESTATE.
 * Refused before any work, with cssm_pf_ll_filter's / cssm_pf_summary's codes: a null handle, t or y and T = 0 (CSSM_EINVAL_ARG), an
 * interval outside (0, 1] (CSSM_EINVAL_ARG).  On an error return the rows are unspecified.
 * The order statistics are exact: a two-rank selection over equal sub-ranges of each row's key range (cssm_intervals.hip), 8 launches
 * per row and the cloud or its keys read 3 times in the ordinary case; its scratch lives on the handle (allocated at the first call,
 * freed by cssm_pf_destroy).  The means are cssm_pf_summary's sums, block for block. */
int cssm_pf_filter_intervals(cssm_pf* pf, const double* t, const double* y, const uint8_t* has_obs, size_t T, double interval,
                             double* ll_out, double* ll_t, int32_t* ess_t,
                             double* state_mean, double* state_lower, double* state_upper,
                             double* eta_of_mean, double* eta_lower, double* eta_upper);
/* The same for T MORE observations of a running filter, as cssm_pf_ll_filter_more continues one: T rows (row s behind record s), no
 * initial row.  CSSM_ESTATE on a handle that was never initialised.  cssm_pf_filter_intervals(t[0..a)) followed by
 * cssm_pf_filter_intervals_more(t[a..T)) gives the rows of cssm_pf_filter_intervals(t[0..T)). */
int cssm_pf_filter_intervals_more(cssm_pf* pf, const double* t, const double* y, const uint8_t* has_obs, size_t T, double interval,
                                  double* ll_out, double* ll_t, int32_t* ess_t,
                                  double* state_mean, double* state_lower, double* state_upper,
                                  double* eta_of_mean, double* eta_lower, double* eta_upper);
/* One streaming step with its row: cssm_pf_step, and the summary of the cloud it leaves, in one call and one synchronisation
 * (state outputs: d doubles each; any may be NULL).  The row has the bits of cssm_pf_summary called behind cssm_pf_step. */
int cssm_pf_step_intervals(cssm_pf* pf, double t, double obs, int has_obs, double interval, double* ll_out, int32_t* ess_out,
                           double* state_mean, double* state_lower, double* state_upper,
                           double* eta_of_mean, double* eta_lower, double* eta_upper);
/* Device time of the last of these three calls on the handle, in milliseconds: ms2[0] the whole call (HIP events around everything it
 * enqueued), ms2[1] the summary launches alone (the GPU's constant 100 MHz clock, stamped by the first block of every row's first
 * launch and read by its last).  CSSM_ESTATE before the first such call has completed. */
int cssm_pf_intervals_last_ms(cssm_pf* pf, double* ms2);

/* One-step-ahead forecasts of ONE large cloud inside the batch filter: ParticleFilter.getMeanForecast mapped over a filter stream
 * (model/ParticleFilter.scala:368-409) -- from every PfState the forecast of the time of the NEXT observation, before that observation
 * is weighed: the prequential check.  The single handle's counterpart of cssm_fleet_filter_forecasts.
 *   The filter part.  t / y / has_obs / T / ll_out / ll_t / ess_t are cssm_pf_ll_filter's arguments bit for bit, and the handle afterwards
 *   (cloud, ancestors, clock, observation index, sums state) is the one it leaves.
 *   The forecast of record s.  T rows laid out like t: state_* [T][d], eta_* / obs_* / obs_below / obs_equal [T]; any of them may be NULL.
 *   Row s is bit for bit -- means and order statistics -- what cssm_pf_forecast(pf, &t[s], 1, keys[s], interval, ...) returns when issued
 *   just before record s is stepped: the source is the cloud before record s through its ancestors (record 0: the initial cloud at
 *   min t); one transition over t[s] - clock on the paired CSSM_STREAM_STEP streams under keys[s], horizon index 0 (dt = 0 allowed);
 *   gamma and eta at t[s]; one observation draw on CSSM_STREAM_OBS; ranks and clamping as documented at cssm_pf_forecast.  The record's
 *   own y plays no part in its row; a record without a datum gets a row like any other.  keys == NULL: keys[s] = cssm_pf_run_key(seed,
 *   2^63 | observation index of the cloud before the record), the rule of thumb of cssm_pf_forecast.
 *   EXTENSION (the reference has none): obs_below[s] / obs_equal[s] = how many of the N drawn observations are strictly below / equal to
 *   y[s] -- the counts of the probability integral transform; both read -1 for a record without a datum and for a NaN row.
 *   A record whose time cssm_pf_forecast would refuse from that cloud (not finite, or before the cloud's time) has a NaN row and counts
 *   of -1; the filter treats the record as cssm_pf_ll_filter does.
 * Refused before any work: a null handle, t or y and T = 0 (CSSM_EINVAL_ARG), an interval outside (0, 1] (CSSM_EINVAL_ARG), a sharded
 * handle (CSSM_ESTATE), and with cssm_pf_forecast's code and message an LGCP handle and a model without the scale its observation draw
 * needs.  On an error return of the filter part the rows are unspecified.  Samples are not offered: cssm_pf_forecast serves a caller who
 * wants them for one state.  Served: the three native resamplers.
 * A row is 8 launches on the handle's stream between the observations' own, no allocation, event or host round trip between records,
 * one synchronisation per call: the forecast kernel in cssm_pf_forecast's geometry (so the means keep its bits), the exact two-rank
 * selection of cssm_pf_filter_intervals over d + 2 rows, a finish; the scratch lives on the handle and is freed by cssm_pf_destroy. */
int cssm_pf_filter_forecasts(cssm_pf* pf, const double* t, const double* y, const uint8_t* has_obs, size_t T,
                             const uint64_t* keys, double interval, double* ll_out, double* ll_t, int32_t* ess_t,
                             double* state_mean, double* state_lower, double* state_upper,
                             double* eta_mean, double* eta_lower, double* eta_upper,
                             double* obs_mean, double* obs_lower, double* obs_upper,
                             int32_t* obs_below, int32_t* obs_equal);
/* The same for T MORE observations of a running filter, as cssm_pf_ll_filter_more continues one (record 0 starts from the handle's cloud
 * at its clock).  CSSM_ESTATE on a handle that was never initialised.  cssm_pf_filter_forecasts(t[0..a)) followed by
 * cssm_pf_filter_forecasts_more(t[a..T)) gives the rows of cssm_pf_filter_forecasts(t[0..T)). */
int cssm_pf_filter_forecasts_more(cssm_pf* pf, const double* t, const double* y, const uint8_t* has_obs, size_t T,
                                  const uint64_t* keys, double interval, double* ll_out, double* ll_t, int32_t* ess_t,
                                  double* state_mean, double* state_lower, double* state_upper,
                                  double* eta_mean, double* eta_lower, double* eta_upper,
                                  double* obs_mean, double* obs_lower, double* obs_upper,
                                  int32_t* obs_below, int32_t* obs_equal);
/* The streaming shape: cssm_pf_step -- t / obs / has_obs / ll_out / ess_out are its arguments and bits -- and, before the record is
 * stepped, cssm_pf_forecast of the single horizon t under `key` (use_key = 0: the rule above with the handle's current observation
 * index), in one call and one synchronisation.  state_* [d], the others one value each; any may be NULL.  CSSM_ESTATE before
 * cssm_pf_init; the other refusals as above. */
int cssm_pf_step_forecast(cssm_pf* pf, double t, double obs, int has_obs, uint64_t key, int use_key, double interval,
                          double* ll_out, int32_t* ess_out,
                          double* state_mean, double* state_lower, double* state_upper,
                          double* eta_mean, double* eta_lower, double* eta_upper,
                          double* obs_mean, double* obs_lower, double* obs_upper,
                          int32_t* obs_below, int32_t* obs_equal);
/* Device time of the last of these three calls on the handle, in milliseconds: ms2[0] the whole call (HIP events around everything it
 * enqueued), ms2[1] the forecast rows' launches alone (the GPU's constant 100 MHz clock, as cssm_pf_intervals_last_ms).  CSSM_ESTATE
 * before the first such call has completed. */
int cssm_pf_forecasts_last_ms(cssm_pf* pf, double* ms2);

/* Forecasts from the current cloud: SimulateData.forecast + summariseForecast (model/Data.scala:196-231) -- the scan of
 * ParticleFilter.getMeanForecast (model/ParticleFilter.scala:389-409) over the future times t[0..H) -- in one call.  The source is
 * exactly the cloud cssm_pf_summary summarises (also between cssm_pf_propagate and cssm_pf_adopt); horizon h starts from the states
 * of horizon h - 1 (h = 0: the cloud, at the handle's time) and
 *   x_h   = stepFunction(t[h] - t[h-1]) of every particle: the transition an unweighted filter step with Philox key `key` and
 *           observation index h draws (CSSM_STREAM_STEP, paired streams) -- dt = 0 allowed;
 *   gamma = f(x_h, t[h]), eta = link(gamma), obs = one draw of mod.observation(gamma) (include/cssm_obs_draws.h, counter
 *           (key, particle, h, CSSM_STREAM_OBS, block)).
 * Per horizon: state_mean[h*d + k] = meanState, state_lower / _upper = getallCredibleIntervals (ranks N - idx - 1, idx - 1);
 * eta_mean / obs_mean = the plain means of the etas and observations (:401-405, not link(f(mean))), eta_ / obs_lower / _upper =
 * getOrderStatistic (ranks N - idx, idx); idx = floor(interval N), ranks clamped to [0, N).  Order statistics are exact (radix
 * selection), means are fp64 block sums.  samples (optional, host): H x (d + 3) x N doubles, row r of horizon h at
 * samples[(h (d + 3) + r) N + i]: the d states, gamma, eta, obs of particle i.  Any output may be NULL.
 * The filter is not touched: cloud, time, observation index, ll, ESS, weights and Philox key stay as they were.
 * Errors: CSSM_ESTATE (not initialised; a sharded handle), CSSM_EINVAL_ARG (interval outside (0, 1]; t not finite, before the
 * cloud's time or decreasing; LGCP, whose observation the reference leaves unimplemented, model/Model.scala:364; a model without
 * the scale its observation needs, with the reference's exception named).  Deviations D10-D12. */
int cssm_pf_forecast(cssm_pf* pf, const double* t, size_t H, uint64_t key, double interval, double* state_mean, double* state_lower,
                     double* state_upper, double* eta_mean, double* eta_lower, double* eta_upper, double* obs_mean, double* obs_lower,
                     double* obs_upper, double* samples);
/* Forecasts from a joint posterior sample p(x, theta | y): SimulateData.forecast(unparamModel, t, n)(s: Rand[(Parameters, State)]) +
 * summariseForecast (model/Data.scala:196-231), the posterior given as M pairs -- theta[m * n_theta ..] in flatten order (cssm_desc_flatten,
 * the theta rows of cssm_pmmh_run*) and x[m * d ..] the state of pair m at time t0 (their last_state rows).  N = the handle's particle
 * count is the reference's n; particle i takes pair pick_i (Streaming.createDist = sampleOne, Resampling.scala:151-154):
 *   pick_i = pick[i] if `pick` is given (N host indices < M), else |int32(word 0 of Philox(key, i, 0, CSSM_STREAM_POST, 0))| mod M
 *            (cssm_posterior_pick, include/cssm_obs_draws.h);
 * and from x[pick_i] at t0 runs cssm_pf_forecast's horizons under theta_{pick_i}: the same normals (CSSM_STREAM_STEP, `key`, horizon h,
 * paired streams) with its own transition coefficients, f(x, t) of the handle's model (f has no parameters), one observation with its own
 * scale (CSSM_STREAM_OBS).  Summaries, samples layout and ranks are cssm_pf_forecast's.  pick_out (optional, N): the pair of each particle.
 * `desc` gives the structure, which must be the handle's (cssm_model_structure words, d, obs_kind, obs_df); each row is written into its
 * parameter slots, validated and constraint-transformed as cssm_pf_set_params would.  The handle only lends its device, stream, contract
 * table and particle count: its cloud, time, parameters, key, ll, ESS and observation index stay as they were (any single-GPU handle,
 * cssm_pfb_chain views included, initialised or not).  The device times land where cssm_pf_forecast_last_ms reads them.
 * Errors: CSSM_ESTATE (sharded handle); CSSM_EINVAL_DESC (structure differs from the handle's); CSSM_EINVAL_ARG (M = 0, n_theta not
 * the descriptor's, a non-finite theta or x entry or a row the model rejects -- naming the row --, pick[i] >= M, interval outside (0, 1],
 * t not finite, before t0 or decreasing; LGCP and models without the scale their observation needs, as cssm_pf_forecast). */
int cssm_pf_forecast_posterior(cssm_pf* pf, const cssm_model_desc* desc, const double* theta, size_t n_theta, const double* x, size_t M,
                               double t0, const double* t, size_t H, const uint32_t* pick, uint64_t key, double interval,
                               double* state_mean, double* state_lower, double* state_upper, double* eta_mean, double* eta_lower,
                               double* eta_upper, double* obs_mean, double* obs_lower, double* obs_upper, double* samples, uint32_t* pick_out);
/* Device time of the last cssm_pf_forecast or cssm_pf_forecast_posterior (HIP events around its kernels), ms2[0] = k_forecast or
 * k_forecast_post, ms2[1] = the radix selection and the finishing kernel, summed over chunks.  CSSM_ESTATE before the first forecast. */
int cssm_pf_forecast_last_ms(cssm_pf* pf, double* ms2);
/* The handle's observation index: the number of observations the current cloud has seen (the default forecast key of the Python
 * mirror is cssm_pf_run_key(seed, 2^63 | this)). */
uint64_t cssm_pf_observation_index(const cssm_pf* pf);
/* mod.observation(gamma).draw on the device for given etas (the `Resample[A]`-like stateless seam of the forecasts):
 * out[i] = the draw of particle i at horizon `step` under `key` -- what cssm_pf_forecast draws for eta[i] -- with the leftmost leaf's
 * stored scale (has_scale, scale) and Student-t's df.  Errors as cssm_pf_forecast's for the model; CSSM_EHIP without a device. */
int cssm_obs_draw(int obs_kind, const double* eta, size_t n, int has_scale, double scale, int df, uint64_t key, uint32_t step,
                  double* out, int device);

/* SimulateData(m).simPompModel(t0) over given times (model/Data.scala:64-73, simStep :186-193; examples/Simulation.scala): n_paths
 * independent realisations of the model itself, drawn on the device.  Stateless, like cssm_obs_draw and cssm_resample.  Time index 0 is
 * t0, time index h >= 1 is t[h - 1]; t finite, not before t0, non-decreasing (dt = 0 allowed).  out (host): (T + 1) x (d + 3) x n_paths
 * doubles in the layout of the forecasts' samples -- row r of time index h for path i at out[(h (d + 3) + r) n_paths + i], the rows
 * being the d states, gamma = f(x, t), eta = link(gamma) and obs = one draw of mod.observation(gamma).
 * Counters (include/cssm_obs_draws.h): x0 of path i is the initial draw of a filter of n_paths particles whose Philox key is `key`
 * (CSSM_STREAM_INIT, id i, step 0, paired streams); the transition into time index h >= 1 and that index's observation use step h - 1 on
 * CSSM_STREAM_STEP (paired streams) / CSSM_STREAM_OBS -- horizon h - 1 of cssm_pf_forecast under the same key; the observation of time
 * index 0 is drawn on CSSM_STREAM_OBS under step CSSM_SIM_STEP_ROW0 = 2^32 - 1.  Hence, for a handle of n_paths particles after
 * cssm_pf_reseed(key) and cssm_pf_init(t0): the states of time index 0 are cssm_pf_get_particles, and time indices 1 .. T are the
 * samples of cssm_pf_forecast(t, T, key, ...), bit for bit.
 * rows_per_launch: time indices one launch covers (0: as many as keep a launch's rows within 1 GiB); the states are carried on the device
 * between launches and the result does not depend on it.
 * Errors, all but the last decided before the first device call, with nothing written to out: CSSM_EINVAL_ARG (null desc / out, null t
 * with T > 0; n_paths outside [1, 2^32 - 2^16]; T >= 2^32 - 1; t0 or a time not finite, a time before t0 or decreasing; LGCP, whose
 * observation the reference leaves unimplemented -- its series come from cssm_simulate_lgcp (simLGCP, by thinning); a model without the scale its
 * observation needs, with the reference's exception named; Student-t with df < 1), CSSM_EINVAL_DESC (a descriptor cssm_pf_create
 * refuses), CSSM_EHIP without a device. */
int cssm_simulate(const cssm_model_desc* desc, uint64_t n_paths, uint64_t key, double t0, const double* t, size_t T, size_t rows_per_launch,
                  int device, double* out);
/* A simulation continued (SimulateData.simMarkov / simRegular in blocks): the paths stand at x (d x n_paths, x[k n_paths + i], finite) at
 * time t0 and move through t[0 .. T); time index j of THIS call moves and draws under step first_step + j, so blocks that hand on their last
 * states and count their steps on are one cssm_simulate.  out: T x (d + 3) x n_paths (no row at t0).  first_step + T must not pass
 * 2^32 - 1.  Errors as cssm_simulate's, and a null or non-finite x. */
int cssm_simulate_from(const cssm_model_desc* desc, uint64_t n_paths, uint64_t key, const double* x, uint32_t first_step, double t0,
                       const double* t, size_t T, size_t rows_per_launch, int device, double* out);
/* Device time (ms, HIP events around its kernels) of the calling thread's last cssm_simulate / cssm_simulate_from; CSSM_ESTATE before one. */
int cssm_simulate_last_ms(double* ms);

/* SimulateData(m).simLGCP(start, end, precision) (model/Data.scala:110-149, simSdeStream :162-176): the event times of a log-Gaussian
 * Cox process by thinning, n_paths independent realisations drawn on the device.  Stateless.  The latent state runs over the grid
 * t_0 = start, t_k = t_(k-1) + delta (delta = 10^-precision, the time accumulated by repeated addition) while
 * t_k <= start + (end - start), every transition with dt = delta exactly; eta_k = exp(f(x_k, t_k)), upper = max_k eta_k; candidates
 * t1 = last + Exponential(upper) from last = start until one passes `end`, each accepted iff V <= eta_k / upper at the largest k with
 * t_k <= t1.  Counters, the index rule and the bounds on a path's work: include/cssm_obs_draws.h (CSSM_STREAM_THIN).  The grid draws
 * are cssm_simulate's: for the same model with Poisson observations, cssm_simulate over the grid times gives the state rows bit for bit
 * wherever t_k - t_(k-1) == delta.  `precision` rules here; desc->lgcp_precision (the filter's) is validated and not used, as the
 * reference takes the two separately.
 * The number of events is not known before the call, so it returns a result object that holds HOST memory only (no device memory
 * outlives the call); the caller reads it into buffers of its own and destroys it:
 *   cssm_lgcp_sim_shape      d, n_paths, grid_points, n_events (all paths);
 *   cssm_lgcp_sim_grid_times t[grid_points];
 *   cssm_lgcp_sim_grid       grid_points x (d + 3) x n_paths in cssm_simulate's layout -- the d states, gamma, eta, obs = 0.0 -- with
 *                            flags & CSSM_LGCP_SIM_KEEP_GRID; without it the rows are never downloaded and this is CSSM_ESTATE;
 *   cssm_lgcp_sim_paths      ev_off[n_paths + 1] (path i owns the events ev_off[i] .. ev_off[i + 1] - 1, in time order), upper[i],
 *                            candidates[i] (those not after `end`), status[i] (CSSM_LGCP_PATH_*: a non-zero path has no events -- the
 *                            reference would throw or not return there -- and the call still succeeds);
 *   cssm_lgcp_sim_events     per event its time, its grid index and its d + 3 values, row-major per event: the states at that index,
 *                            gamma, eta and 1.0.
 * Any output pointer may be NULL.  The reference's vector of one path is its events newest first, then its grid points in time order.
 * paths_per_launch: paths one pair of launches covers (0: as many as keep the grid rows on the device within 1 GiB), rounded up to a
 * whole number of pairs of paths; the result does not depend on it.
 * Errors, all but the last two decided before the first device call, *out untouched: CSSM_EINVAL_ARG (null desc / out; n_paths outside
 * [1, 2^32 - 2^16]; precision outside [0, 9]; start or end not finite, end < start; a model that is not CSSM_OBS_LGCP -- cssm_simulate
 * draws those; more than 2^24 grid points; a grid whose d + 3 rows for one pair of paths exceed 1 GiB; unknown flags),
 * CSSM_EINVAL_DESC (a descriptor cssm_pf_create refuses), CSSM_ENOMEM, CSSM_EHIP without a device. */
typedef struct cssm_lgcp_sim cssm_lgcp_sim;
#define CSSM_LGCP_SIM_KEEP_GRID 1
int cssm_simulate_lgcp(const cssm_model_desc* desc, uint64_t n_paths, uint64_t key, double start, double end, int precision, int flags,
                       size_t paths_per_launch, int device, cssm_lgcp_sim** out);
int cssm_lgcp_sim_shape(const cssm_lgcp_sim* sim, int* d, uint64_t* n_paths, uint64_t* grid_points, uint64_t* n_events);
int cssm_lgcp_sim_grid_times(const cssm_lgcp_sim* sim, double* t);
int cssm_lgcp_sim_grid(const cssm_lgcp_sim* sim, double* rows);
int cssm_lgcp_sim_paths(const cssm_lgcp_sim* sim, uint64_t* ev_off, double* upper, uint32_t* candidates, int32_t* status);
int cssm_lgcp_sim_events(const cssm_lgcp_sim* sim, double* ev_t, uint32_t* ev_idx, double* ev_rows);
void cssm_lgcp_sim_destroy(cssm_lgcp_sim* sim);
/* Device time (ms, HIP events) of the calling thread's last cssm_simulate_lgcp: ms2[0] its grid kernels, ms2[1] its thinning launches
 * (the counting and the writing one); CSSM_ESTATE before a call. */
int cssm_simulate_lgcp_last_ms(double* ms2);

/* FilterInterpolate (model/ParticleFilter.scala:273-311, ParticleFilter.interpolate :335-337): the filter whose
 * particles are whole paths, so that a weighted step resamples the paths and missing observations are
 * interpolated by the surviving lineages.  The forward pass keeps the history of clouds and ancestor arrays on the
 * device ((T+1) * N * (8 d + 4) bytes); the output is, for every time index s = 0..T (0 = initial cloud), the
 * summary examples/Interpolate.scala:42-44 forms from the transposed paths of the LAST state: mean, the
 * getCredibleInterval order statistics and eta (see cssm_pf_summary).  Arrays: (T+1)*d doubles (state_*),
 * T+1 doubles (eta_*); any may be NULL.  The handle must be re-initialised before further streaming calls.
 * flags: CSSM_INTERP_REFERENCE_PAIRING pairs output entry k with the cloud of time index T - k (evaluated with
 * the time of index k): what the example's `(interpolated, interpolated.last.particles.transpose).zipped` really
 * does, since the transposed paths run newest-first; 0 gives the chronological pairing the example intends. */
#define CSSM_INTERP_REFERENCE_PAIRING 1
int cssm_pf_interpolate(cssm_pf* pf, const double* t, const double* y, const uint8_t* has_obs, size_t T, double interval,
                        int flags, double* ll_out, double* state_mean, double* state_lower, double* state_upper,
                        double* eta_of_mean, double* eta_lower, double* eta_upper);
/* ---- EXTENSION (not a restatement of running reference code: the reference has no smoother beyond FilterInterpolate): forward filtering,
 * backward simulation of ONE series on a cloud of any size the handle holds -- cssm_fleet_smooth (below) for the single handle, whose
 * backward kernels tile the SLOTS over many workgroups instead of keeping a cloud inside one.  The forward pass is cssm_pf_interpolate's
 * (the same code, history and ll_out bits); then n_traj trajectories are drawn backwards through the kept clouds under the contract's
 * backward kernel (include/cssm_numerics.h, "backward simulation") with seed = the handle's Philox key, and summarised per time index.
 * Per time index, going back, launches on the handle's stream: the level (per trajectory and tile of CSSM_SMOOTH_TILE slots, then folded
 * over the tiles), the exact 128-bit sums of the weights per tile, and the search (tile, then slot); an index whose record has a
 * component with sd not > 0 takes the genealogical step in one launch.
 *
 * t / y / has_obs / T, the T + 1 output rows (row 0 the initial cloud; row s is time index s) and the handle's state afterwards are
 * cssm_pf_interpolate's: its own buffers hold no cloud, it must be re-initialised before further streaming calls.  Row s summarises
 * the n_traj states the trajectories hold at index s: the mean is their plain fp64 sum / n_traj, lower / upper the order statistics at
 * the ranks cssm_pf_summary takes for n_traj values, eta as cssm_fleet_smooth forms it.  Any output may be NULL.  traj_out (may be
 * NULL): [T + 1][n_traj], entry [row][m] the particle of slice `row` (an index into the cloud that record proposed, < N) trajectory m
 * passes through.  1 <= n_traj <= CSSM_FLEET_MAX_N and flags must be 0 (CSSM_INTERP_REFERENCE_PAIRING is refused by name), else
 * CSSM_EINVAL_ARG; an LGCP handle is CSSM_EINVAL_ARG (its transition over an event is a chain of sub-steps, not one Gaussian), a sharded
 * one CSSM_ESTATE; every resampler is served.  History or work space that does not fit is CSSM_ENOMEM naming the bytes. */
int cssm_pf_smooth(cssm_pf* pf, const double* t, const double* y, const uint8_t* has_obs, size_t T,
                   uint32_t n_traj, double interval, int flags, double* ll_out,
                   double* state_mean, double* state_lower, double* state_upper,
                   double* eta_of_mean, double* eta_lower, double* eta_upper,
                   uint32_t* traj_out);
/* ms3 = device time (HIP events on the handle's stream) of the forward pass, of the backward simulation and of the row summaries of the
 * last cssm_pf_smooth.  CSSM_ESTATE before the first.  The array holds THREE doubles. */
int cssm_pf_smooth_last_ms(cssm_pf* pf, double* ms3);

/* ---- EXTENSION (the reference has no likelihood maximiser): iterated filtering for ONE swarm of any size the handle holds -- one search
 * of cssm_fleet_if2 (below), whose swarm ends at CSSM_FLEET_MAX_N particles because a workgroup keeps it.  Here the particles are tiled
 * over many workgroups (CSSM_IF2_TILE a block), the swarm lives in device memory as theta[2][n_theta][N] beside x[2][d][N], and what needs
 * a value of the whole cloud is a launch of its own: 5 launches per weighted record, 1 per unweighted one, 3 per iteration (cssm_if2.hip),
 * all enqueued ahead on the handle's stream with one synchronisation per call.  The arithmetic is the contract's (include/
 * cssm_numerics.h, "iterated filtering"): bit for bit a one-series cssm_fleet_if2 where that exists, and the sequential twin beyond.
 *
 * The semantics are those of one series of cssm_fleet_if2.  Start: theta0[n_theta] or swarm0[n_theta][N] (wins when both are given).
 * Iteration first_iter + q runs under cssm_pf_run_key(seed, first_iter + q + 1) and cools by cssm_fleet_if2_cooling.  Outputs:
 * theta_mean[n_iters][n_theta], ll[n_iters]; optional swarm_out[n_theta][N]; optional, of the last iteration: ll_t[T], ess_t[T],
 * x_out[d][N] (the cloud the last record proposed), anc_out[N].  A record that leaves no particle a usable weight ends the search:
 * CSSM_ENONFINITE, rows from the failing iteration on read NaN, swarm_out is the swarm that iteration started from, the last-iteration
 * outputs read NaN / -1 / 0xffffffff.  T = 0 leaves everything untouched: the rows read NaN, CSSM_OK.  A search continued from swarm_out
 * with first_iter = the iterations done is bit for bit the uninterrupted one.
 *
 * The handle is only LENT: its device, stream, contract table, N and the structure of the descriptor it was created with.  Its parameter
 * values are not read; cloud, ancestors, clock, key, window ring, options and ll / ess are afterwards what they were.  The search keeps
 * buffers of its own, allocated up front: N (24 n_theta + 16 d + 16) + ceil(N / CSSM_IF2_TILE) (48 + 8 n_theta) bytes and the rows;
 * CSSM_ENOMEM names the bytes if they do not fit.
 * Refused before the handle is looked at (CSSM_EINVAL_ARG): null rw_sd, theta_mean or ll; null t / y with T > 0; theta0 and swarm0 both
 * null; a negative or non-finite rw_sd; n_iters outside [1, 1000000] or first_iter + n_iters beyond 2^31; a cooling fraction outside
 * (0, 1]; a null handle.  Then: an LGCP handle (CSSM_EINVAL_ARG, by name), a sharded handle (CSSM_ESTATE), a handle whose
 * CSSM_OPT_RESAMPLER is not systematic (CSSM_ESTATE, naming the option: the contract's search resamples systematically), n_theta other
 * than the handle's descriptor flattens to (CSSM_EINVAL_ARG).  A refused call leaves a handle that filters as before. */
#define CSSM_IF2_TILE 1024u
int cssm_pf_if2(cssm_pf* pf, const double* theta0, const double* swarm0, size_t n_theta,
                const double* rw_sd, double cooling_fraction_50, uint32_t first_iter, uint32_t n_iters,
                uint64_t seed, const double* t, const double* y, const uint8_t* has_obs, size_t T,
                double* theta_mean, double* ll, double* swarm_out, double* ll_t, int32_t* ess_t,
                double* x_out, uint32_t* anc_out);
/* *ms = device time of the launches of the last cssm_pf_if2 (HIP events on the handle's stream); CSSM_ESTATE before the first. */
int cssm_pf_if2_last_ms(cssm_pf* pf, double* ms);

/* ---- fixed-lag interpolation of a live handle: FilterInterpolate as the stream it is (ParticleFilter.interpolate, model/
 * ParticleFilter.scala:281-310 -- one stepInterpolate per observation, every element carrying the paths that survive to that moment;
 * examples/Interpolate.scala: once data resumes behind a gap, the surviving lineages fill it) for ONE cloud of any size the handle
 * holds.  The semantics are those of cssm_fleet_window / cssm_fleet_step_interpolate (below), for one series.
 *
 * cssm_pf_window(pf, slices): the handle remembers its `slices` most recent clouds and the ancestor arrays that resampled them in a ring
 * on the device -- slices x stride x (8 d + 4) bytes and one uint32[N] index array (about 470 MB at N = 2^20, d = 3, 16 slices).
 * slices >= 2 allocates and sets the depth to 0 (re-opening, with the same size or another, restarts the window); 0 frees; 1 is
 * CSSM_EINVAL_ARG.  An allocation that does not fit is CSSM_ENOMEM naming the bytes (counted without overflow; a count beyond the
 * device's memory is refused without allocating), and the handle goes on without a window.  cssm_pf_destroy frees the ring.  A sharded
 * handle is CSSM_ESTATE, an LGCP handle refused in cssm_pf_interpolate's words.
 * cssm_pf_window_depth(pf): the records remembered behind the base slice, 0 .. slices - 1 (the base slice is not counted; a full ring
 * overwrites its oldest slice and the depth stays slices - 1); 0 for a null handle or no window.
 *
 * cssm_pf_step_interpolate: cssm_pf_step -- t / obs / has_obs / ll_out / ess_out, their bits, the hold-and-redo of an observation and
 * the handle left afterwards (cloud, ancestors, clock, observation index, level state) are exactly cssm_pf_step's -- which also copies
 * the cloud the step proposed and the ancestors that resampled it (a record without a datum: none, the identity) into the window's newest
 * slot, behind the step's own launches, with the slice's time; and, unless lag == CSSM_PF_NO_ROWS, returns the last min(lag, depth) + 1
 * time indices through the lineages that survive to the cloud just written, row 0 the newest: per row 8 launches (k_lineage_fill, which
 * composes the lineage one slice further back and fills the selection's keys in one pass; the six passes of the exact two-rank
 * selection; k_iv_finish), no allocation, event or read-back between the rows, one synchronisation per call as cssm_pf_step_intervals.
 *   Outputs: state_* = [lag + 1][d], eta_* = [lag + 1]; any may be NULL.  For a handle stepped through records 0 .. m by this call only,
 *   its window open since before record 0, row j (0 <= j <= min(lag, depth)) is bit for bit row m + 1 - j of cssm_pf_interpolate over
 *   records 0 .. m (flags 0, the same t0, parameters, key and resampler), the means included; row 0 therefore has the bits of
 *   cssm_pf_summary behind the step.  Rows min(lag, depth) < j <= lag read NaN; rows_out = min(lag, depth) + 1, or 0 under
 *   CSSM_PF_NO_ROWS, where nothing of the rows is written.  The bounded ring changes no row it still returns: the lineages are only ever
 *   composed from the newest index back.  The f coefficients of a row are F(t) of its slice's time.
 *   Continuity: the window is continuous only across consecutive cssm_pf_step_interpolate calls.  Every other call that writes the
 *   handle's cloud, key or parameters (cssm_pf_init, _init_from, _step, _step_intervals, _step_forecast, _propagate, _adopt, _ll_filter,
 *   _ll_filter_more, _filter, _filter_intervals(_more), _filter_forecasts(_more), _interpolate, _smooth, cssm_pmmh_run, _reseed,
 *   _set_params, _set_option(CSSM_OPT_RESAMPLER)) sets the depth to 0, and the next cssm_pf_step_interpolate first records the cloud the
 *   handle holds then (what cssm_pf_get_particles returns, identity ancestors) as the base slice at the handle's clock: the rows never
 *   reach behind it.  Calls that only read (cssm_pf_summary, _forecast, _forecast_posterior, _get_*) leave the window alone.  An open
 *   window changes nothing any other call returns.  A call that fails after the step has begun restarts the window.
 *   Errors, before any work: a null handle and an interval outside (0, 1] are CSSM_EINVAL_ARG; a sharded handle CSSM_ESTATE; an LGCP
 *   handle cssm_pf_interpolate's refusal; a handle without a window CSSM_ESTATE naming cssm_pf_window; a lag >= slices other than
 *   CSSM_PF_NO_ROWS CSSM_EINVAL_ARG naming both numbers; a handle that is not initialised cssm_pf_step's CSSM_ESTATE.
 * cssm_pf_step_interpolate_last_ms: ms2[0] = device time of the whole last call (an event pair round everything it enqueued), ms2[1] =
 * of its row launches alone (the GPU's constant 100 MHz clock, as cssm_pf_intervals_last_ms; 0 without rows); CSSM_ESTATE before the
 * first call on the window.  The array holds TWO doubles. */
#define CSSM_PF_NO_ROWS 0xffffffffu
int cssm_pf_window(cssm_pf* pf, uint32_t slices);
uint32_t cssm_pf_window_depth(const cssm_pf* pf);
int cssm_pf_step_interpolate(cssm_pf* pf, double t, double obs, int has_obs, uint32_t lag, double interval,
                             double* ll_out, int32_t* ess_out, uint32_t* rows_out,
                             double* state_mean, double* state_lower, double* state_upper,
                             double* eta_of_mean, double* eta_lower, double* eta_upper);
int cssm_pf_step_interpolate_last_ms(cssm_pf* pf, double* ms2);

/* ---- stateless resampler: the `Resample[A]` seam (model/package.scala:23) ------------------ */

/* Resampling.systematicResampling (model/Resampling.scala:63-72) on host arrays: weights w[n]
 * (the unnormalised w1 = exp(w - max) the reference passes, :125-126), one uniform u in [0,1),
 * anc[n] receives the index of the particle that slot i copies.  Runs on `device`. */
int cssm_resample_systematic(const double* w, size_t n, double u, uint32_t* anc, int device);
/* The same seam for every resampler the library has: kind = CSSM_RESAMPLE_SYSTEMATIC (reads u; seed and step unused),
 * CSSM_RESAMPLE_STRATIFIED (model/Resampling.scala:78-86) or CSSM_RESAMPLE_MULTINOMIAL (:92-96), whose per-slot uniforms
 * come from the Philox streams of (seed, step) -- the ancestors a filter with that seed selects at observation `step`
 * for the same weights (u unused).  The reference draws them from unseeded global generators (:66, :83, :93). */
int cssm_resample(int kind, const double* w, size_t n, double u, uint64_t seed, uint32_t step, uint32_t* anc, int device);
/* EXTENSION -- not a drop-in for running reference code: Resampling.residualResampling (model/Resampling.scala:130-146) cannot run as
 * written (it hands Vector.range(1, m) with n weights to the multinomial resampler, indexes the particles with what comes back, and
 * exp-normalises weights that stepFilter has already exponentiated).  This is the resampler its scaladoc describes (:124-129): particle
 * i appears k_i = floor(n w_i / sum w) times, in particle order, and the remaining m = n - sum k_i slots are drawn by multinomial
 * resampling on the residual weights n w_i / sum w - k_i (the draws of cssm_resample(CSSM_RESAMPLE_MULTINOMIAL): one uniform per slot
 * from the Philox stream of (seed, step)).  anc[s] = the particle slot s takes: first the copies, then the m draws in draw order.
 * Arithmetic: csrc/cssm_residual.hip; oracle twin: oracle_resample_residual. */
int cssm_resample_residual(const double* w, size_t n, uint64_t seed, uint32_t step, uint32_t* anc, int device);

/* ---- sharded filter: stage calls between which the caller runs its collectives ------------ */
/*
 * EXACT exchange, one observation on R ranks -- LGCP series, forced, or the repetition of a series an
 * outlying observation voided:
 *   cssm_pf_shard_propagate     fused propagate + weight + fixed-point sums of exp(w - c) on the local shard, c being
 *                               the observation's reference level (cssm_numerics.h: known without any exchange);
 *                               5 x u64 out: S, S2 (2 words each), order key of the local max log-weight
 *   [all-gather of 5 x u64 per rank -- the only collective before the resampling exchange]
 *   cssm_pf_shard_offspring     global max -> was c usable?  If so: global cumulative weights -> end slot of every
 *                               local particle; ll, ess; for every destination rank q the range of local particles
 *                               that own at least one slot of q: first[R], count[R]; *redo_flag = 0.
 *                               If not (outlying observation; always for LGCP): *redo_flag = 1 and the caller runs
 *   cssm_pf_shard_sums          local sums again, relative to the max taken from the gathered words: 5 x u64
 *   [all-gather of 5 x u64 per rank]  and cssm_pf_shard_offspring once more
 *   [all-to-all of count[R], all-to-all-v of (d+1) doubles per particle]
 *   cssm_pf_shard_pack / _adopt pack the send ranges of the OTHER ranks (a rank's own range never
 *                               travels); adopt the rows received from lower (n_low) and higher
 *                               (n_high) ranks around the own range and expand to the N_local slots
 * All device work is enqueued on the stream given at creation; the only host reads are the
 * ones whose pointers are documented as host (the caller reads count[R] and the flag in one copy).
 */
int cssm_pf_shard_init(cssm_pf* pf, double t0);
int cssm_pf_shard_propagate(cssm_pf* pf, double t, double obs, int has_obs, uint64_t* sums5_dev);
int cssm_pf_shard_sums(cssm_pf* pf, const uint64_t* all_sums5_dev, int world, uint64_t* sums5_dev);
int cssm_pf_shard_offspring(cssm_pf* pf, const uint64_t* all_sums5_dev, int rank, int world,
                            int64_t* send_first_dev, int64_t* send_count_dev, uint64_t* redo_flag_dev);
int cssm_pf_shard_pack(cssm_pf* pf, int world, const int64_t* send_first_host,
                       const int64_t* send_count_host, int skip_rank, double* send_buf_dev);
int cssm_pf_shard_adopt(cssm_pf* pf, const double* recv_buf_dev, int64_t n_low, int64_t n_high,
                        int64_t self_first, int64_t self_count);
int cssm_pf_shard_result(cssm_pf* pf, double* ll_out, int32_t* ess_out);

/* A series known in advance: the records of all T observations are uploaded once (cssm_pf_shard_begin) and observation s is
 * propagated by cssm_pf_shard_propagate_at(s) (in order; sums5_dev as above, or NULL when the single-collective exchange
 * totals the sums itself).  cssm_pf_shard_status at the end: ll, ess and the sticky bits -- 4: the max ruled some
 * observation's reference level out (run the series again with the exact exchange), 8: a capacity miss that was not resumed;
 * need[s] = rows observation s needed (diagnostics). */
int cssm_pf_shard_begin(cssm_pf* pf, const double* t, const double* y, const uint8_t* has_obs, size_t T);
/* (measurement) What one block of every exchange launch of the peer-written exchange spent polling its peers since the cloud was drawn, as of
 * the last cssm_pf_shard_status: out4 = {exchanges counted, ticks the first offspring block waited for every rank's header words, ticks
 * the first expansion block waited for them, ticks it then waited for its neighbours' eager-rows flags}; ticks of the GPU's constant
 * 100 MHz clock.  At world 1 a block waits for its own launch's header block; across GPUs a slow link or a late peer shows up here and
 * not in the kernels' durations.  bench.py reports the per-exchange means (per_rank.header_wait_us, rows_wait_us). */
int cssm_pf_shard_wait_stats(cssm_pf* pf, uint64_t* out4);

/* T MORE observations of the sharded filter that is already running -- what cssm_pf_ll_filter_more is to a single-GPU handle
 * (Flow.scan(init)(stepFilter) handed the next T elements, model/ParticleFilter.scala:163-166): no new cloud, the first time
 * increment from the handle's clock, record s of the call = observation (observations so far + s) of the filter.  Steps,
 * exchanges, cssm_pf_shard_status and cssm_pf_shard_resume then address the call's records 0 .. T-1 as after _begin. */
int cssm_pf_shard_continue(cssm_pf* pf, const double* t, const double* y, const uint8_t* has_obs, size_t T);
int cssm_pf_shard_propagate_at(cssm_pf* pf, size_t s, uint64_t* sums5_dev);
int cssm_pf_shard_status(cssm_pf* pf, double* ll_out, int32_t* ess_out, uint32_t* bits_out, uint32_t* need, size_t T);
/* `filter` on shards (model/ParticleFilter.scala:152-158): with cssm_pf_shard_want_path(pf, 1) set BEFORE cssm_pf_shard_begin /
 * _continue, the rank that owns the GLOBAL slot sampleOne picks after an observation (Resampling.scala:151-154; the index is a
 * function of seed and observation, the same on every rank) records the state in that slot.  cssm_pf_shard_get_path copies
 * this rank's (T + 1) x d rows to the host: row s + 1 = the pick after observation s of the series (row 0: of the initial cloud;
 * all zero after _continue), rows of slots other ranks own are all-zero bits -- the caller combines the ranks' paths (exactly
 * one is non-zero per row; ShardedFilter.filter sums the 32-bit halves of the bit patterns). */
int cssm_pf_shard_want_path(cssm_pf* pf, int on);
int cssm_pf_shard_get_path(cssm_pf* pf, double* out_host, size_t T);

/* getIntervals (model/ParticleFilter.scala:415-424; cssm_pf_summary above) of the SHARDED cloud.  The order statistics are
 * ranks in the global cloud of n_global particles, so every radix-selection pass totals the ranks' byte histograms with one
 * all-reduce; the means are the all-reduced local sums over n_global.  Stage calls, the same on every rank:
 *   cssm_pf_shard_summary_begin(pf, interval, sums_dev, hist_dev)   keys of this rank's resampled cloud (d state rows +
 *                           eta = link(f(x, t))); sums_dev[d] <- local sums of the state components; hist_dev zeroed
 *   for shift = 56, 48, ..., 0:
 *     cssm_pf_shard_summary_hist(pf, shift, hist_dev)               local byte histograms of the still-matching keys
 *     [caller: all-reduce SUM of hist_dev, (d + 1) * 512 uint32]
 *     cssm_pf_shard_summary_pick(pf, shift, hist_dev)               every rank picks the same byte; hist_dev zeroed again
 *   [caller: all-reduce SUM of sums_dev]
 *   cssm_pf_shard_summary_finish(pf, sums_dev, ...)                 outputs as cssm_pf_summary (host pointers, may be NULL)
 * sums_dev (d doubles) and hist_dev ((d + 1) * 512 uint32) are DEVICE buffers of the caller (the ones its collective
 * works on); all launches go to the handle's stream.  Order statistics are exact (equal to the single-GPU filter's
 * over the concatenated shards); the means agree with it to ~1e-13 relative (another order of summation). */
int cssm_pf_shard_summary_begin(cssm_pf* pf, double interval, double* sums_dev, uint32_t* hist_dev);
int cssm_pf_shard_summary_hist(cssm_pf* pf, int shift, uint32_t* hist_dev);
int cssm_pf_shard_summary_pick(cssm_pf* pf, int shift, uint32_t* hist_dev);
int cssm_pf_shard_summary_finish(cssm_pf* pf, const double* sums_global_dev, double* state_mean, double* state_lower, double* state_upper,
                                 double* eta_of_mean, double* eta_lower, double* eta_upper);

/* SINGLE-COLLECTIVE exchange (every weighted observation of an ordinary series): ONE all-to-all per observation carries
 * the rank's 5 sum words (segment header, to every rank) AND its boundary particles -- to the rank below its first `cap`
 * particles, to the rank above its last `cap`, each with the inclusive prefix of its fixed-point weight within that block --
 * so no all-gather precedes it and the host reads nothing.  The receiver, holding every rank's sums after the exchange,
 * turns the prefixes into global end slots itself.  Slots of a rank owned neither by its own particles nor by the adjacent
 * ranks' boundary blocks raise sticky bit 8 (a capacity miss).
 *   cssm_pf_shard_spec_segment    doubles per pair of ranks for capacity `cap` (send / recv buffers: world segments)
 *   cssm_pf_shard_propagate_at    with sums5_dev = NULL
 *   [level from the global max instead (LGCP; repetition after an outlying observation): propagate_at with sums5_dev,
 *    all-gather of the 5 words, cssm_pf_shard_sums -- the sums are then relative to the level the gathered max selects]
 *   cssm_pf_shard_boundary_pack   a header for every destination, boundary rows for the two adjacent ranks
 *   (all-to-all of cssm_pf_shard_spec_segment doubles per pair)
 *   cssm_pf_shard_adopt_spec      offspring of the own particles, expansion of the received rows, coverage check
 * recv_buf_dev must stay untouched until the next propagate has run (ancestors point into it). */
int64_t cssm_pf_shard_spec_segment(const cssm_pf* pf, int64_t cap);
/* Particles per unit sum of this shard (a whole number of 1024-particle tiles).  A capacity that is a multiple of it lets
 * cssm_pf_shard_boundary_pack take the totals and prefixes of the boundary blocks from the unit sums instead of forming them
 * again (any capacity is correct; ShardedFilter rounds up to it). */
int64_t cssm_pf_shard_unit(const cssm_pf* pf);
int cssm_pf_shard_boundary_pack(cssm_pf* pf, int rank, int world, int64_t cap, double* send_buf_dev);
int cssm_pf_shard_adopt_spec(cssm_pf* pf, const double* recv_buf_dev, int rank, int world, int64_t cap);
/* A capacity miss is resumable.  The launch that found some rank's slots uncovered did nothing on any rank (every rank
 * reaches the same verdict from the segment headers), recorded the observation index and sticky bit 8, and every later
 * kernel of the series returned at once.  cssm_pf_shard_resume returns that index, clears the bit and rewinds the handle to
 * "that observation propagated, not yet resampled"; the host redoes its exchange with a larger capacity (boundary_pack,
 * all-to-all, adopt_spec) and continues the series behind it. */
int cssm_pf_shard_resume(cssm_pf* pf, uint32_t* fail_step_out);
/* ... and so is an observation whose reference level its max rules out (sticky bit 4: an outlying datum; the launch that found out
 * resampled nothing, recorded the observation, every later kernel returned at once).  cssm_pf_shard_resume_level returns its index,
 * clears the bit and rewinds the handle to "that observation NOT yet propagated" (its source cloud is untouched); the host runs it
 * again with the level taken from the all-gathered max (cssm_pf_shard_propagate_at with sums5_dev, cssm_pf_shard_sums, then the
 * exchange) and continues behind it -- also inside a continued series, which cannot be repeated from its start. */
int cssm_pf_shard_resume_level(cssm_pf* pf, uint32_t* fail_step_out);

/* The single-collective series with its collectives driven from INSIDE the library (RCCL over xGMI, resolved at run time
 * with dlopen: the copy already in the process, else librccl.so of the ROCm installation).  Per weighted observation s in
 * [s_begin, s_end): propagate_at -> boundary_pack -> ONE RCCL all-to-all -> adopt_spec, everything enqueued on the handle's
 * stream, no host wait.  single_collective = 1: equal-split ncclAllToAll of whole segments; 2: ncclAllToAllv in which only
 * the adjacent pairs exchange whole segments and every other pair the 12 header words (nothing else of those segments is
 * ever read; falls back to 1 when world <= 2 or the RCCL copy has no ncclAllToAllv); 3 = the same for any world, an error
 * without ncclAllToAllv (tests); + 4 (i.e. 5, 6, 7): the level of every observation comes from the GLOBAL max -- an
 * ncclAllGather of the ranks' 5 words and cssm_pf_shard_sums precede the all-to-all (LGCP series, whose level IS the max;
 * the repetition of a series an outlying observation voided): 2 collectives per observation, still no host read.
 * The communicator is made from an id that rank 0 creates and hands to the other ranks by
 * whatever channel the host has (bench.py: torch.distributed's object broadcast).  weighted[s] != 0: observation s
 * resamples.  Buffers (device): send / recv world * cssm_pf_shard_spec_segment doubles each; sums5 (5 words) / all_sums5
 * (5 * world words) are used by the + 4 modes only.
 * The library never waits without a bound for work that contains its collectives: cssm_pf_shard_status / _resume poll the
 * stream, watch the communicator's asynchronous error state and after CSSM_SHARD_TIMEOUT_S seconds (environment; default
 * 600) abort the communicator and return CSSM_ERCCL -- a rank that died or returned early surfaces as an error on every
 * rank instead of a hang.  A rank whose own RCCL call fails aborts the communicator before returning, for the same reason. */
typedef struct { char internal[128]; } cssm_rccl_id;   /* ncclUniqueId */
int cssm_rccl_available(void);
const char* cssm_rccl_library(void);   /* which librccl.so the library bound to (diagnostics) */
int cssm_rccl_unique_id(cssm_rccl_id* id_out);
int cssm_rccl_comm_create(const cssm_rccl_id* id, int world, int rank, int device, void** comm_out);
void cssm_rccl_comm_destroy(void* comm);
int cssm_pf_shard_series_rccl(cssm_pf* pf, void* comm, int rank, int world, size_t s_begin, size_t s_end,
                              const uint8_t* weighted, int64_t cap, uint64_t* sums5_dev, uint64_t* all_sums5_dev,
                              double* send_buf_dev, double* recv_buf_dev, int single_collective);

/* PEER-WRITTEN exchange: the same single-collective protocol without a collective.  Every rank owns two receive windows (they
 * alternate by exchange) and a flag per (window, source rank) in ONE slab of device memory that the other ranks map
 * (hipIpcOpenMemHandle across processes -- one process per GPU over xGMI peer access; the plain pointer where several shards share
 * a process, and for the rank itself).  k_boundary_pack writes segment (rank -> q) -- header, and for the two adjacent ranks the
 * boundary rows -- straight into q's window and, when the last of its blocks has made its stores visible at system scope, stores the
 * exchange number into q's flag (release); q's k_offspring_expand_spec polls the flags of all ranks (acquire, bounded: a rank that
 * never delivers raises a device error instead of hanging the GPU) before it reads a header.  Two launches per weighted
 * observation -- propagate, then pack + offspring + expansion in one (the pack blocks lead the grid) -- and nothing else: no RCCL
 * launch, no host wait.  The windows hold the
 * capacity they were set up for; an exchange that is resumed with a larger capacity, and observations whose level comes from the
 * global max, go through the collective exchange above (the two share every kernel and produce the same bits).
 *   cssm_pf_shard_peer_setup    allocate this rank's slab for (world, cap); *mine_out = what the other ranks need to map it
 *   [the host exchanges the handles: every rank receives all `world` of them, in rank order]
 *   cssm_pf_shard_peer_connect  map them, build the device table
 *   cssm_pf_shard_series_peer   observations [s_begin, s_end) of the resident series (cssm_pf_shard_begin / _continue), or stage
 *                               by stage: cssm_pf_shard_propagate_at(s, NULL), cssm_pf_shard_pack_peer, cssm_pf_shard_pack_rows_peer,
 *                               cssm_pf_shard_adopt_peer
 *   cssm_pf_shard_peer_close    unmap and free (also done by cssm_pf_destroy)
 * model/ParticleFilter.scala:116-132 is the step whose resampling this exchange completes across GPUs. */
typedef struct cssm_peer_handle {
  char ipc[64];          /* hipIpcMemHandle_t of the slab (valid if has_ipc) */
  uint64_t pid;          /* owner process: a rank of the same process uses local_ptr instead of the IPC handle */
  uint64_t local_ptr;    /* the slab's address in the owner's process */
  uint64_t bytes;        /* size of the slab: equal on all ranks (same world, capacity and latent dimension) */
  int32_t device, has_ipc;
} cssm_peer_handle;
int cssm_pf_shard_peer_setup(cssm_pf* pf, int rank, int world, int64_t cap, cssm_peer_handle* mine_out);
int cssm_pf_shard_peer_connect(cssm_pf* pf, const cssm_peer_handle* all_handles, int world);
/* One empty round of the protocol -- every rank writes a (non-zero) token into every rank's flags and waits, bounded, for everybody's
 * in its own -- called by all ranks at the same point right after connecting: a mapping, peer access or cross-GPU visibility that does
 * not work surfaces here, as CSSM_ESHARD on the host, before a series depends on it. */
int cssm_pf_shard_peer_handshake(cssm_pf* pf, uint32_t token);
/* (round 5) The handshake also carries a PAYLOAD: every rank stores 16 probe words (a function of token, source rank and index) at the
 * head of its segment in every peer's window 0 ahead of its token, the way the exchange's pack blocks store rows; a second launch behind
 * the handshake reads what the peers left in this rank's window with system-scope loads -- what every kernel of the library reads a
 * window with -- and CSSM_ESHARD names how many words read wrongly.  The same words read with PLAIN loads are counted too and reported
 * here (diagnostic: a line some cache of this GPU kept from an earlier round; not on any data path).  Callers run two rounds with
 * different tokens, a host barrier between them. */
uint32_t cssm_pf_shard_peer_probe_stale(const cssm_pf* pf);
void cssm_pf_shard_peer_close(cssm_pf* pf);
int cssm_pf_shard_pack_peer(cssm_pf* pf, int rank, int world, int64_t cap);
/* (round 5) EAGER ROWS + NEEDED ROWS.  A boundary block holds `cap` rows (sized for the worst observation, ~6 sqrt(N_global)), a typical
 * observation's neighbour needs a few hundred of them, and every row is a remote store over one xGMI link.  The rows next to the boundary
 * (CSSM_PEER_EAGER_ROWS, default 4096 = four tiles) are written AT ONCE, with a flag of their own that is long set when the reader gets to
 * them.  Rows beyond them travel only if the neighbour's slots need them: once the headers of all ranks are there the SENDER can tell
 * (end slot beyond its own last slot / run starting below its own first slot: the reader's arithmetic), so the pack's row blocks wait for
 * the headers, write those rows and publish their number behind a second flag -- which the reader waits for only when the eager rows do
 * not reach its first / last slot (it sees that from the eager rows).  In stage-by-stage use the rows beyond the eager ones are a stage of
 * their own: cssm_pf_shard_pack_peer (headers + eager rows) on every shard, cssm_pf_shard_pack_rows_peer on every shard,
 * cssm_pf_shard_adopt_peer on every shard.  CSSM_PEER_ALL_ROWS=1 (read when the handle is created), or an eager count >= the capacity:
 * every row travels at once, pack_rows_peer does nothing.
 * cssm_pf_shard_peer_rows: rows written for neighbours / neighbour segments / segments that needed rows beyond the eager ones, so far
 * (diagnostics; beyond_out may be NULL). */
int cssm_pf_shard_pack_rows_peer(cssm_pf* pf, int rank, int world, int64_t cap);
int cssm_pf_shard_peer_rows(cssm_pf* pf, uint64_t* rows_out, uint64_t* segments_out, uint64_t* beyond_out);
/* Diagnostics for a series that ended in "a rank's segment did not arrive": this rank's flag words of both windows (world x 96 uint32 each:
 * per source rank [0] header flag, [16] eager rows flag, [17] needed rows, [18] flag of the rows beyond the eager ones, [32..79] the 24
 * self-validating header words), its 256 local ticket words and the handle's exchange counter; returns the words written (< 0: error). */
int64_t cssm_pf_shard_peer_debug(cssm_pf* pf, uint32_t* out, size_t nwords);
int cssm_pf_shard_adopt_peer(cssm_pf* pf, int rank, int world, int64_t cap);
/* pack + adopt in ONE launch (the pack blocks lead the grid): for a rank that has its stream to itself, i.e. one process per GPU --
 * what cssm_pf_shard_series_peer enqueues.  Shards that share a stream use the stage calls, every stage on all shards before the next. */
int cssm_pf_shard_exchange_peer(cssm_pf* pf, int rank, int world, int64_t cap);
int cssm_pf_shard_series_peer(cssm_pf* pf, int rank, int world, size_t s_begin, size_t s_end, const uint8_t* weighted, int64_t cap);

/* ---- PMMH host loop ---------------------------------------------------------------------- */
/*
 * ParticleMetropolisHastings (model/PMMH.scala:68-81,114-123) with proposal
 * Parameters.perturb(delta) (model/Parameters.scala:65-67), a symmetric transition (0) and a
 * flat prior (0), as examples/DetermineParameters.scala:59,73 wires it.  theta0[n_theta] is
 * the flattened STORED parameter vector in Parameters.flattenParams order
 * (model/Parameters.scala:88-95: per leaf scale-if-present, then m0, c0, [mu|phi...] in
 * SdeParameter.flatten order).  Each iteration re-parameterises the handle, reseeds it with
 * cssm_pf_run_key(seed, iteration + 1), runs `filter`, and accepts iff log(u) < ll' - ll (initial ll = -1e99).
 * Outputs, one row per iteration (the stream drops the initial state, :97): ll[n_iters],
 * theta[n_iters * n_theta], accepted[n_iters] (running count), last_state[n_iters * d].
 */
int cssm_pmmh_run(cssm_pf* pf, const cssm_model_desc* desc, const double* theta0, size_t n_theta,
                  double delta, const double* t, const double* y, const uint8_t* has_obs, size_t T,
                  uint64_t seed, size_t n_iters, double* ll, double* theta, int32_t* accepted,
                  double* last_state);

/* ---- batched independent filters ------------------------------------------------------------ */
/*
 * B filters of ONE model structure -- the chains of a PMMH run (examples/DetermineParameters.scala:68-69 runs two under mapAsync(2)),
 * the parameter grid of a pilot run (model/Streaming.scala:38-39: mapAsyncUnordered(4)) -- advanced in lockstep: one launch per stage
 * for all of them (grid.y = the chain), enqueued by ONE host thread.  At N = 100 000 particles a single filter leaves most of the GPU
 * idle and a step is launch latency + one wave's dependent instruction stream; B chains cost little more than one.
 *   cssm_pfb_create          B handles of `desc`'s structure and n_particles each, on one stream
 *   cssm_pfb_filter          `filter` (model/ParticleFilter.scala:152-158) of chain k under descs[k] (same structure) and the Philox key
 *                            seeds[k]: ll_out[k], path_out[k][(T + 1) * d] (may be NULL), rc_out[k] = that chain's own status
 *                            (CSSM_ENONFINITE: its weights were unusable).  Per chain the bits of cssm_pf_reseed + cssm_pf_filter on a
 *                            handle of its own: a chain the batched launches do not serve (an observation ruled out of its reference
 *                            level, LGCP, another resampler) is run through that very driver.
 *   cssm_pmmh_run_batched    cssm_pmmh_run (model/PMMH.scala:68-81,114-123) for B chains in lockstep -- chain k from theta0[k * n_theta ..]
 *                            under seeds[k]: the same proposals, filter keys and decisions as B separate runs, every iteration's B
 *                            filters as one batch.  Outputs chain-major: ll[k * n_iters + it], theta[(k * n_iters + it) * n_theta + j],
 *                            accepted[k * n_iters + it], last_state[(k * n_iters + it) * d + j].
 *   cssm_pfb_chain           chain k as an ordinary handle (inspection: particles, ancestors, summaries); owned by the batch.
 */
typedef struct cssm_pfb cssm_pfb;
int cssm_pfb_create(const cssm_model_desc* desc, uint64_t n_particles, int n_chains, int device, cssm_pfb** out);
void cssm_pfb_destroy(cssm_pfb* b);
int cssm_pfb_num_chains(const cssm_pfb* b);
cssm_pf* cssm_pfb_chain(cssm_pfb* b, int k);
int cssm_pfb_filter(cssm_pfb* b, const cssm_model_desc* const* descs, const uint64_t* seeds, const double* t, const double* y,
                    const uint8_t* has_obs, size_t T, double* ll_out, double* path_out, int* rc_out);
int cssm_pmmh_run_batched(cssm_pfb* b, const cssm_model_desc* desc, const double* theta0, size_t n_theta, double delta, const double* t,
                          const double* y, const uint8_t* has_obs, size_t T, const uint64_t* seeds, size_t n_iters, double* ll, double* theta,
                          int32_t* accepted, double* last_state);
/* (round 5) ONE chain at two iterations per batch: a batch of three filters holds iteration i's proposal and BOTH candidates for iteration
 * i + 1 (its proposal from iteration i's proposal, and from the current parameters): the proposals and filter keys are functions of
 * (seed, iteration, parameters) alone, so they can be drawn and filtered before iteration i has decided.  Output identical to
 * cssm_pmmh_run(seed), bit for bit; `b` holds exactly three chains (a batch that fails is redone candidate by candidate in the sequential order: the same result on the error paths too).  At N = 100 000 a single filter leaves most of the GPU idle: three
 * cost little more than one (model/PMMH.scala:68-81). */
int cssm_pmmh_run_speculative(cssm_pfb* b, const cssm_model_desc* desc, const double* theta0, size_t n_theta, double delta, const double* t,
                              const double* y, const uint8_t* has_obs, size_t T, uint64_t seed, size_t n_iters, double* ll, double* theta,
                              int32_t* accepted, double* last_state);

/* Number of stored parameters of a descriptor and their copy-out / copy-in in flatten order. */
int cssm_desc_flatten(const cssm_model_desc* desc, double* theta, size_t cap, size_t* n_theta);

/* Diagnostic: the structure words the kernels branch on (one byte per latent component: SDE kind | place in the f map << 2 |
 * leaf ends << 4 | leftmost leaf << 5; four components per word, CSSM_MAX_DIM / 4 words) and the latent dimension.  The models
 * whose words are listed in csrc/cssm_prop.hip (KnownStructures) run kernels that hold them at compile time. */
int cssm_model_structure(const cssm_model_desc* desc, uint32_t* words_out, int32_t* d_out);

/* ---- fleet of independent series ------------------------------------------------------------
 * The reference's everyday shape: a streaming filter per sensor (filterStream, model/ParticleFilter.scala:163-166) over many
 * sensors, N = 100 ... 2000 particles each (examples/Filtering.scala:24, examples/DetermineParameters.scala, the pilot run of
 * model/Streaming.scala:19-40).  A cssm_fleet holds S series of ONE model structure (the cssm_model_structure words, d, obs_kind,
 * obs_df of the descriptor it is created with), N particles each; parameters, Philox key, data and clock are every series' own.
 * One launch advances all of them, ONE WORKGROUP PER SERIES: a cloud of at most CSSM_FLEET_MAX_N particles keeps its weights, its
 * scan and its ancestors in the workgroup's LDS, so nothing of a series crosses a block ("Fleet").
 *
 * Per series k every result has the bits of a handle of its own -- cssm_pf_create(descs[k], N, seeds[k]) driven through the same
 * calls -- and so of the oracle: ll, ll_t, ess_t, cloud, ancestors, observation index, the paired Philox streams.
 *
 * Served: every observation model, every transition and composition, d = 1 .. CSSM_MAX_DIM, systematic resampling,
 * 1 <= N <= CSSM_FLEET_MAX_N.  The LGCP observation model (sub-stepped events, FilterLgcp) is asked for by name, as the reference asks
 * for FilterLgcp by name: cssm_fleet_create_lgcp makes the fleet, cssm_fleet_create keeps refusing an LGCP descriptor.  An LGCP fleet
 * serves _destroy, _num_series, _num_particles, _set_params, _reseed, _set_option, _init, _init_from, _step, _ll_filter, _ll_filter_more, _filter,
 * _summary, _get_particles, _get_ancestors, _observation_index, _last_ms and _pmmh_chains_lgcp (whole PMMH chains over its event streams;
 * _pmmh_chains keeps refusing it by name); every other call on it is CSSM_EINVAL_ARG before anything runs.
 * Everything else is refused at cssm_fleet_create / _set_params / _set_option with CSSM_EINVAL_ARG /
 * CSSM_EINVAL_DESC and a message naming the reason and the entry points that do serve it (cssm_pf_*, cssm_pfb_*); a fleet call
 * never degenerates into S single-handle runs.  Thread-affinity and device rules as for every entry point: each call selects the
 * fleet's device; the fleet owns a non-blocking stream; a fleet is not re-entrant.
 * Not here: sharded fleets, other resamplers. */
typedef struct cssm_fleet cssm_fleet;
/* 12 bytes of LDS per particle (weight 8, ancestor 4) + 7.3 KB per block: 55.3 KB at 4096, two blocks per CU of 160 KiB; the summary
 * kernel sorts a row of at most 4096 keys (32 KiB) in LDS. */
#define CSSM_FLEET_MAX_N 4096

/* Errors: CSSM_EINVAL_ARG (N outside [1, CSSM_FLEET_MAX_N], S = 0, device out of range), CSSM_EINVAL_DESC (invalid descriptor,
 * LGCP), CSSM_EHIP (no device), CSSM_ENOMEM (16 d N bytes of state per series). */
int cssm_fleet_create(const cssm_model_desc* desc, uint64_t n_particles, uint32_t n_series, int device, cssm_fleet** out);
/* A fleet of LGCP event streams: FilterLgcp(mod, resample, precision) (model/ParticleFilter.scala:169-227) for S streams, the bits of
 * cssm_pf_* under an LGCP descriptor per stream.  desc->obs_kind must be CSSM_OBS_LGCP -- anything else is CSSM_EINVAL_DESC naming
 * cssm_fleet_create, decided before any device is touched; desc->lgcp_precision is part of the fleet's structure (a cssm_fleet_set_params
 * descriptor of another precision is CSSM_EINVAL_DESC naming the series).  N, S, device and memory limits and errors as cssm_fleet_create.
 * Data: every record is an event -- y and has_obs are ignored and may be NULL, the step always weighs; an event at the time of the one
 * before it (dt == 0) takes no sub-step, weighs gamma - gamma and keeps the state; the sub-step clock, and f at the sub-step times of a
 * seasonal leaf, are the handle's.  Per-series statuses are the plain fleet's (CSSM_ENONFINITE ends one series, an empty series is
 * CSSM_EINVAL_ARG, CSSM_ESTATE without a cloud).  Not served, CSSM_EINVAL_ARG with a message that says "LGCP fleet" and names what
 * serves the request: _filter_intervals, _filter_intervals_more, _step_intervals, _filter_forecasts, _step_forecast, _forecast, _forecast_posterior, _interpolate,
 * _window, _step_interpolate, _simulate, _pmmh_run.  Intervals of a stream: cssm_fleet_summary after a step. */
int cssm_fleet_create_lgcp(const cssm_model_desc* desc, uint64_t n_particles, uint32_t n_series, int device, cssm_fleet** out);
void cssm_fleet_destroy(cssm_fleet* f);
uint32_t cssm_fleet_num_series(const cssm_fleet* f);
uint64_t cssm_fleet_num_particles(const cssm_fleet* f);
/* descs[k] = the parameters of series k (pointers may repeat); every descriptor must have the fleet's structure, else
 * CSSM_EINVAL_DESC naming the series, and the fleet keeps the parameters it had.  Until the first call every series has the
 * parameters of the creating descriptor. */
int cssm_fleet_set_params(cssm_fleet* f, const cssm_model_desc* const* descs);
/* seeds[k] = the Philox key of series k (default 0).  Derive the keys of one user seed with cssm_pf_run_key(seed, k). */
int cssm_fleet_reseed(cssm_fleet* f, const uint64_t* seeds);
/* CSSM_OPT_RESAMPLER, and only CSSM_RESAMPLE_SYSTEMATIC: any other resampler is CSSM_EINVAL_ARG with the reason (the
 * `Resample[A]` a FilterFleet is constructed with goes through here); CSSM_OPT_FORECAST_CAP (KiB, 0 = 1 GiB, negative refused): the
 * samples cssm_fleet_forecast / cssm_fleet_forecast_posterior hold on the device at a time; CSSM_OPT_FLEET_SELECT; CSSM_OPT_INTERP_CAP
 * (KiB, 0 = 1 GiB, negative refused): the lineage history cssm_fleet_interpolate holds on the device at a time.  Every other option
 * is CSSM_EINVAL_ARG. */
int cssm_fleet_set_option(cssm_fleet* f, int option, int value);

/* llFilter (model/ParticleFilter.scala:137-140) of every series, ragged: series k owns the records off[k] .. off[k+1]-1 of
 * t / y / has_obs (off[0] = 0, non-decreasing, S + 1 entries; has_obs may be NULL = all 1); its cloud is drawn afresh at the
 * slice's smallest time (data.minBy(_.t)).  ll_out[S]; ll_t / ess_t (optional) laid out like t; rc_out[S] = the series' OWN status:
 * CSSM_OK; CSSM_EINVAL_ARG for a series with no records (the reference's minBy throws; the series is left as it was);
 * CSSM_ENONFINITE when its weights were unusable at some observation -- its cloud is then undefined until it is initialised again
 * (the rule of cssm_pf_step), its later records are skipped (their ll_t / ess_t read NaN / -1, ll_out[k] NaN), and every other
 * series is bit for bit what it is without it.  The call returns non-zero only for errors that are not one series' own
 * (CSSM_EINVAL_ARG: null arguments, off[0] != 0 or off decreasing; HIP failures).  A fleet continues with cssm_fleet_step
 * afterwards as a handle does after cssm_pf_ll_filter. */
int cssm_fleet_ll_filter(cssm_fleet* f, const uint64_t* off, const double* t, const double* y, const uint8_t* has_obs,
                         double* ll_out, double* ll_t, int32_t* ess_t, int* rc_out);

/* filter (model/ParticleFilter.scala:152-158) of every series: cssm_fleet_ll_filter -- the same arguments, the same ll_out / ll_t /
 * ess_t / rc_out, the same cloud, ancestors, clock and observation index left behind (the fleet continues with cssm_fleet_step) -- and
 * the sampled path (Resampling.sampleOne, model/Resampling.scala:151-154), recorded by the series' own workgroup inside the one launch.
 *   path_out (may be NULL): series k owns rows off[k] + k .. off[k+1] + k, T_k + 1 rows of d doubles (off[S] + S rows in all).  Row 0
 *     is the initial cloud's particle at slot abs((int32)Philox(seed_k, 0, 0, CSSM_STREAM_PICK, 0).v[0]) % N, row s + 1 the resampled
 *     particle at the record's pick after observation s (identity ancestors behind an observation without a datum).
 *   last_out (may be NULL): [S][d], row T_k of series k's path -- what a Metropolis chain keeps.  With last_out alone the device keeps
 *     and the host reads S x d doubles, not the paths.
 * Per series every result is bit for bit cssm_pf_reseed + cssm_pf_filter on a handle of its own.  At least one of path_out and last_out
 * must be given: with neither the call is CSSM_EINVAL_ARG and names cssm_fleet_ll_filter.  Errors as cssm_fleet_ll_filter; a series that
 * fails with CSSM_ENONFINITE keeps the rows recorded before the failing observation (rows 0 .. s for a failure at observation s), its
 * later rows and its last_out row read NaN; a series with no records (CSSM_EINVAL_ARG) has NaN in its single row; no other series
 * notices either.  Null off / ll_out / rc_out / data, both outputs NULL and off[0] != 0 are refused before the fleet is looked at. */
int cssm_fleet_filter(cssm_fleet* f, const uint64_t* off, const double* t, const double* y, const uint8_t* has_obs,
                      double* ll_out, double* ll_t, int32_t* ess_t, double* path_out, double* last_out, int* rc_out);

/* The reference's everyday program (examples/Filtering.scala:24-31: filter, then getIntervals of every emitted PfState,
 * model/ParticleFilter.scala:415-424) of every series: cssm_fleet_ll_filter -- off / t / y / has_obs / ll_out / ll_t / ess_t / rc_out are
 * its arguments bit for bit, and the cloud, ancestors, clock and observation index left behind are the ones it leaves (the fleet
 * continues with cssm_fleet_step) -- and cssm_fleet_summary of the initial cloud and of the cloud after every record, written by the
 * series' own workgroup inside the ONE launch: no history, no second launch, no device memory beyond the outputs.
 *   Rows are laid out like cssm_fleet_filter's path_out: series k owns rows off[k] + k .. off[k+1] + k (T_k + 1 rows, off[S] + S in
 *   all); row 0 is the initial cloud at the slice's smallest time, row s + 1 the cloud after observation s (identity ancestors behind an
 *   observation without a datum), eta with F at the row's own time.  state_mean / state_lower / state_upper: [off[S] + S][d];
 *   eta_of_mean / eta_lower / eta_upper: [off[S] + S]; any of the six may be NULL.
 * Order statistics exact, ranks and clamping as cssm_pf_summary documents them (a state row and the eta row take different rank pairs),
 * means plain fp64 sums, eta_of_mean = link(f(mean, t)) formed on the host.  Every row is preset to NaN: a series with no records
 * (CSSM_EINVAL_ARG) has NaN in its single row; a series that fails with CSSM_ENONFINITE at observation s keeps rows 0 .. s and reads NaN
 * from row s + 1 on; no other series notices either.  Null off / ll_out / rc_out / t / y, off[0] != 0, an interval outside (0, 1] and
 * a null fleet are refused with CSSM_EINVAL_ARG before the fleet is looked at; a decreasing off as by cssm_fleet_ll_filter.  The device
 * time is cssm_fleet_last_ms()[0]. */
int cssm_fleet_filter_intervals(cssm_fleet* f, const uint64_t* off, const double* t, const double* y, const uint8_t* has_obs,
                                double interval, double* ll_out, double* ll_t, int32_t* ess_t,
                                double* state_mean, double* state_lower, double* state_upper,
                                double* eta_of_mean, double* eta_lower, double* eta_upper, int* rc_out);

/* ParticleMetropolisHastings (model/PMMH.scala:68-81,114-123; examples/DetermineParameters.scala) for S chains in lockstep, a chain
 * per series, ONE launch per iteration: chain k starts at theta0[k * n_theta ..], runs under seeds[k] and sees series k's slice of the
 * data (off / t / y / has_obs as cssm_fleet_ll_filter; the slices may repeat one data set or differ per sensor).  Per iteration:
 * cssm_pmmh_run's proposal and filter key for every chain, cssm_fleet_set_params, cssm_fleet_reseed, one cssm_fleet_filter with
 * last_out only, cssm_pmmh_run's decision for every chain; a chain whose filter is CSSM_ENONFINITE is rejected (ll' = -inf), any other
 * status ends the run with it.  Outputs chain-major as cssm_pmmh_run_batched: ll[k * n_iters + it], theta[(k * n_iters + it) * n_theta
 * + j], accepted[...], last_state[(k * n_iters + it) * d + j].  Chain k is bit for bit cssm_pmmh_run(handle of N particles, theta0[k],
 * its slice, seeds[k]).  The fleet's parameters and keys are those of the last iteration afterwards.
 * Refused: null arguments, off[0] != 0, an LGCP descriptor (CSSM_EINVAL_DESC), n_theta that is not the descriptor's -- all before the
 * fleet is looked at --, off decreasing, an empty slice (CSSM_EINVAL_ARG, before the first iteration), a descriptor of another
 * structure than the fleet's (CSSM_EINVAL_DESC).  What a fleet does not hold (LGCP, other resamplers, N > CSSM_FLEET_MAX_N) is refused
 * at cssm_fleet_create / _set_option as ever; cssm_pmmh_run_batched serves those. */
int cssm_fleet_pmmh_run(cssm_fleet* f, const cssm_model_desc* desc, const double* theta0, size_t n_theta, double delta,
                        const uint64_t* off, const double* t, const double* y, const uint8_t* has_obs,
                        const uint64_t* seeds, size_t n_iters,
                        double* ll, double* theta, int32_t* accepted, double* last_state);
/* Where the last cssm_fleet_pmmh_run spent its time, milliseconds summed over its iterations: ms6[0] proposals + set_params + reseed
 * (host), [1] record building (host), [2] upload and [3] kernel (HIP events), [4] decisions (host); ms6[5] = the iterations counted. */
int cssm_fleet_pmmh_last_split(cssm_fleet* f, double* ms6);

/* initialiseState + stepFilter (:105-132).  cssm_fleet_init draws every series' cloud at its own t0[k].  cssm_fleet_step advances
 * the series with active[k] != 0 (active NULL = every series) by one observation (t[k], y[k], has_obs[k]; has_obs NULL = all 1): the
 * bits of cssm_pf_step.  Inactive series are untouched (their t / y / has_obs entries are not read, their ll_out / ess_out entries
 * not written, rc_out[k] = CSSM_OK).  rc_out[k] = CSSM_ENONFINITE as above; CSSM_ESTATE for an active series without a cloud
 * (never initialised, or failed since).  The call returns CSSM_ESTATE when no series of the fleet has a cloud. */
int cssm_fleet_init(cssm_fleet* f, const double* t0);
int cssm_fleet_step(cssm_fleet* f, const uint8_t* active, const double* t, const double* y, const uint8_t* has_obs,
                    double* ll_out, int32_t* ess_out, int* rc_out);

/* FilterInit(mod, resample, initState).initialiseState (model/ParticleFilter.scala:252-271) of the series with active[k] != 0 (active NULL =
 * every series), and its posterior form: the clouds come from the caller.  Series k owns the rows moff[k] .. moff[k+1]-1 of x, d doubles
 * each in flatten order, M_k of them (moff[0] = 0, non-decreasing, S + 1 entries, as in cssm_fleet_forecast_posterior).
 *   M_k = 1: the row replicated N times -- for every call that follows the series has the bits of cssm_pf_init_from(t0[k], row) on a handle
 *     of its own under the same key and parameters.
 *   M_k > 1: particle i starts at row pick_i of the series' rows; pick_i = pick[k * N + i] when pick ([S][N], optional) is given, otherwise
 *     cssm_posterior_pick(keys[k], i, M_k) (include/cssm_obs_draws.h) -- the selection cssm_fleet_forecast_posterior makes under the same
 *     keys, so a filter started this way stands on the cloud that forecast stands on.  With neither pick nor keys the series is refused.
 *   pick_out (optional, [S][N]) receives the picks; the rows of series that are inactive or refused read 0.
 * A served series is left with identity ancestors, ll = 0, ess = N, clock t0[k], observation index 0, its window restarted (a call that
 * writes a series' cloud: cssm_fleet_step_interpolate, Continuity) and, in an LGCP fleet, no predicted level -- what cssm_fleet_init leaves,
 * but for the cloud.  LGCP fleets are served.  Inactive series are untouched: cloud, clock, window, rc_out[k] = CSSM_OK; their t0, rows and
 * picks are not read -- unlike cssm_fleet_init the call can restart some sensors while the others keep streaming.
 * rc_out[S] = the series' OWN status: CSSM_EINVAL_ARG, the series left exactly as it was and cssm_last_error naming the first such series,
 * for M_k = 0 on an active series, a non-finite t0[k] or row entry, a pick >= M_k, the missing keys above.  Null t0 / moff / x / rc_out,
 * moff[0] != 0 and a null fleet are refused with CSSM_EINVAL_ARG before the fleet is looked at; a decreasing moff (S is the fleet's) before
 * anything of the fleet is changed.  ONE launch without records, as cssm_fleet_init's; the device time is cssm_fleet_last_ms()[0]. */
int cssm_fleet_init_from(cssm_fleet* f, const uint8_t* active, const double* t0, const uint64_t* moff, const double* x,
                         const uint32_t* pick, const uint64_t* keys, uint32_t* pick_out, int* rc_out);

/* ---- EXTENSION (not a restatement of running reference code: the reference has no online parameter learner -- its ParamFilterState,
 * model/ParticleFilter.scala:89-94, is never used -- and nothing there writes one filter's cloud from another's): whole series copied
 * between the series of one fleet, or from a second fleet of the same shape, on the device.  It is what SMC2 (composablestatespacemodels_amd/
 * smc2.py: Chopin, Jacob and Papaspiliopoulos 2013) needs of a fleet whose series are its parameter particles: resampling them
 * (series k <- series a[k]) and adopting the freshly filtered cloud of a proposal fleet.
 *
 * map has cssm_fleet_num_series(dst) entries; src may be dst.  An entry is a SIGNED 64-bit number (an int64_t in two's complement: -1 is
 * CSSM_FLEET_COPY_KEEP) in the unsigned 64-bit type every other index array of the fleet section has -- an int64_t array is passed as it
 * is, with a cast.  The assignment is SIMULTANEOUS: every read sees the state before the call,
 * so a rotation, a swap and "everybody from series 0" are well defined.  For map[k] = j >= 0 with a source series j that has a cloud,
 * series k of dst afterwards holds series j's cloud (cssm_fleet_get_particles is bit-equal; it sits in the half of state[S][2][d][n] that
 * j's observation index selects), ancestors, ll, ess and (LGCP fleet) predicted level, clock, observation index (Philox counter word and
 * buffer parity), liveness and parameters (the parameter block is uploaded again before the next launch) -- and j's Philox key only under
 * CSSM_FLEET_COPY_KEYS: by default the destination keeps its own.  Series k's window restarts (a call that writes a series' cloud:
 * cssm_fleet_step_interpolate, Continuity); the source's is untouched.  map[k] = CSSM_FLEET_COPY_KEEP, and map[k] = k with src == dst,
 * leave series k entirely untouched (rc_out[k] = CSSM_OK).
 *   Continuity: after the call every fleet call on dst series k has the bits of a series that was created with series j's parameters and
 *   key, driven through series j's calls and then -- unless CSSM_FLEET_COPY_KEYS -- given series k's key by cssm_fleet_reseed
 *   (cssm_pf_reseed on a handle of its own).
 * rc_out[S] = the series' OWN status: CSSM_ESTATE when the source series has no cloud (never initialised, or failed since) -- the
 * destination is then left exactly as it was and cssm_last_error names the first such series.  Refused for the whole call, before anything
 * changes: CSSM_EINVAL_ARG for a null dst / src / map / rc_out (before either fleet is looked at), a map entry outside [-1, S_src), unknown
 * flag bits, another N, another device, one fleet LGCP and the other not; CSSM_EINVAL_DESC for another model structure (the
 * cssm_model_structure words, obs_kind, obs_df, lgcp_precision: the message names what differs).  LGCP fleets are served: no record and
 * no transition is touched.
 * One gather kernel over (moved series x tiles of a cloud), k_fleet_copy; kept, self-mapped and dead-source series get no block.  From a
 * second fleet: one launch, ordered behind the source fleet's stream by an event.  Within one fleet nothing waits on another block; the
 * call stages instead: the first launch writes every moved cloud into the destination's own NON-live half -- nobody reads one, so any
 * map is free of conflicts -- and the ancestors and scalars into scratch; a second launch settles, within each series, the clouds whose
 * required half is the other one and brings ancestors and scalars home.  The device time is cssm_fleet_last_ms()[0]. */
#define CSSM_FLEET_COPY_KEEP (-1)   /* map entry: leave the series exactly as it is */
#define CSSM_FLEET_COPY_KEYS 1      /* flags: the Philox key travels too (default: the destination keeps its own key) */
int cssm_fleet_copy_series(cssm_fleet* dst, cssm_fleet* src, const uint64_t* map, int flags, int* rc_out);

/* cssm_pf_ll_filter_more for every series: T_k MORE records of the filters that are already running, in ONE launch -- what a loop of T
 * cssm_fleet_step calls does with a launch and a host round trip per record.  off / t / y / has_obs / ll_t / ess_t are laid out as in
 * cssm_fleet_ll_filter.  No cloud is drawn; the first increment of a series is taken from its clock, and record s of the call is
 * observation (cssm_fleet_observation_index(f, k) + s) of the series -- the Philox counter word and the key of its resampling uniform, as
 * cssm_fleet_step packs its one record: cssm_fleet_ll_filter(t[0..a)) followed by cssm_fleet_ll_filter_more(t[a..T)) leaves the bits of
 * cssm_fleet_ll_filter(t[0..T)), and so does the loop of cssm_fleet_step.  ll_out[k] is the log-likelihood accumulated since the series
 * was initialised.  rc_out[S] = the series' OWN status: a series without records is untouched (CSSM_OK, ll_out[k] not written -- the
 * inactive series of cssm_fleet_step); one with records but no cloud gets CSSM_ESTATE and is untouched (its ll_t / ess_t read NaN / -1);
 * CSSM_ENONFINITE at record s as in cssm_fleet_ll_filter (later records skipped, NaN / -1, ll_out[k] NaN, the cloud undefined until the
 * series is initialised again, no other series notices).  A series the call advances restarts its window.  The call returns CSSM_ESTATE
 * when no series of the fleet has a cloud.  LGCP fleets are served (y / has_obs may be NULL there).  Null off / ll_out / rc_out / data,
 * off[0] != 0 and a null fleet are refused with CSSM_EINVAL_ARG before the fleet is looked at; a decreasing off as by
 * cssm_fleet_ll_filter.  The device time is cssm_fleet_last_ms()[0]. */
int cssm_fleet_ll_filter_more(cssm_fleet* f, const uint64_t* off, const double* t, const double* y, const uint8_t* has_obs,
                              double* ll_out, double* ll_t, int32_t* ess_t, int* rc_out);

/* cssm_fleet_ll_filter_more -- the same arguments, bits and statuses -- and cssm_fleet_summary of the cloud after every record, from the
 * same launch.  There is no row for an initial cloud, since none is drawn: series k owns rows off[k] .. off[k+1]-1, laid out like t, preset
 * to NaN; state_mean / state_lower / state_upper: [off[S]][d]; eta_of_mean / eta_lower / eta_upper: [off[S]]; any of the six may be NULL.
 * Order statistics, ranks, clamping, means and eta_of_mean are those of cssm_fleet_filter_intervals.  A series that fails at record s keeps
 * the rows of the records before it; one without a cloud reads NaN.  An LGCP fleet is refused as by cssm_fleet_filter_intervals; null
 * off / ll_out / rc_out / t / y, off[0] != 0, an interval outside (0, 1] and a null fleet are refused with CSSM_EINVAL_ARG before the fleet
 * is looked at. */
int cssm_fleet_filter_intervals_more(cssm_fleet* f, const uint64_t* off, const double* t, const double* y, const uint8_t* has_obs,
                                     double interval, double* ll_out, double* ll_t, int32_t* ess_t,
                                     double* state_mean, double* state_lower, double* state_upper,
                                     double* eta_of_mean, double* eta_lower, double* eta_upper, int* rc_out);

/* The streaming shape of cssm_fleet_filter_intervals (filterStream, then getIntervals of every state; one observation per sensor per
 * call): cssm_fleet_step -- the same arguments, bits and statuses -- and cssm_fleet_summary of every cloud the call moved, from the same
 * launch.  state_* [S][d], eta_* [S], any may be NULL; the entries of a series that is inactive, has no cloud (CSSM_ESTATE) or fails
 * (CSSM_ENONFINITE) are not written, as its ll_out / ess_out entries are not.  Null t / y / rc_out, an interval outside (0, 1] and a null
 * fleet are refused with CSSM_EINVAL_ARG before the fleet is looked at.  The device time is cssm_fleet_last_ms()[0]. */
int cssm_fleet_step_intervals(cssm_fleet* f, const uint8_t* active, const double* t, const double* y, const uint8_t* has_obs,
                              double interval, double* ll_out, int32_t* ess_out,
                              double* state_mean, double* state_lower, double* state_upper,
                              double* eta_of_mean, double* eta_lower, double* eta_upper, int* rc_out);

/* One-step-ahead forecasts inside the filtering launch: ParticleFilter.getMeanForecast mapped over a filter stream
 * (model/ParticleFilter.scala:368-409) -- from every PfState the forecast of the time of the NEXT observation, before that observation
 * is weighed: the prequential check of a filtered sensor -- of every series, in ONE launch.
 *   The filter part.  off / t / y / has_obs / ll_out / ll_t / ess_t / rc_out are cssm_fleet_ll_filter's arguments bit for bit, and the
 *   cloud, ancestors, clock, observation index and statuses left behind are the ones it leaves.
 *   The forecast of record r.  Outputs are laid out like t: R = off[S] rows, state_* [R][d], eta_* / obs_* / obs_below / obs_equal [R]; any
 *   of them may be NULL.  Row r is bit for bit what cssm_fleet_forecast returns for that series with the single horizon t[r] under key
 *   keys[r], issued just before the record is stepped: the source is the series' cloud before record r through its ancestors (the
 *   initial cloud at the slice's smallest time for the first record); one transition over t[r] - clock on the paired CSSM_STREAM_STEP
 *   streams under keys[r], horizon index 0 (dt = 0 allowed); gamma and eta at t[r] under the series' own parameters; one observation draw
 *   on CSSM_STREAM_OBS with the series' own scale; ranks and clamping as documented at cssm_pf_forecast, order statistics exact, means
 *   plain fp64 sums in cssm_fleet_forecast's order.  The record's own y plays no part in its row; a record without a datum gets a row
 *   like any other.  keys == NULL: keys[r] = cssm_pf_run_key(seed_k, 2^63 | observation index of the cloud before the record), the rule of
 *   thumb of cssm_fleet_forecast.
 *   EXTENSION (the reference has none): obs_below[r] / obs_equal[r] = how many of the N drawn observations are strictly below / equal to
 *   y[r] -- the counts of the probability integral transform; both read -1 for a record without a datum and for a NaN row.
 *   Statuses.  Every row is preset to NaN.  A series that fails with CSSM_ENONFINITE at record s keeps rows 0 .. s (row s is formed before
 *   the weighing) and reads NaN from row s + 1 on.  A record whose time is not finite or lies before the series' clock has a NaN row --
 *   cssm_fleet_forecast refuses such a time --, and the filter treats the record as cssm_fleet_ll_filter does.  fc_rc_out[S] (required) is
 *   the forecast's own status: CSSM_OK, or CSSM_EINVAL_ARG for a series whose model lacks the scale its observation draw needs: every
 *   forecast row of that series is NaN, its filter results are untouched, and cssm_last_error carries the reference's exception for the
 *   first such series although the call succeeds.  No other series notices any of this.
 * Samples are not offered here: at fleet scale they are R (d + 3) N doubles, and cssm_fleet_forecast serves a caller who wants them for
 * one state.  Null off / t / y / ll_out / rc_out / fc_rc_out, off[0] != 0, an interval outside (0, 1] and a null fleet are refused with
 * CSSM_EINVAL_ARG before the fleet is looked at; a decreasing off as by cssm_fleet_ll_filter.  The device time is cssm_fleet_last_ms()[0]. */
int cssm_fleet_filter_forecasts(cssm_fleet* f, const uint64_t* off, const double* t, const double* y, const uint8_t* has_obs,
                                const uint64_t* keys, double interval, double* ll_out, double* ll_t, int32_t* ess_t,
                                double* state_mean, double* state_lower, double* state_upper,
                                double* eta_mean, double* eta_lower, double* eta_upper,
                                double* obs_mean, double* obs_lower, double* obs_upper,
                                int32_t* obs_below, int32_t* obs_equal, int* rc_out, int* fc_rc_out);
/* The streaming shape of cssm_fleet_filter_forecasts (one observation per sensor per call): cssm_fleet_step -- active / t / y / has_obs /
 * ll_out / ess_out / rc_out are its arguments, bits and statuses -- and, before the record is stepped, cssm_fleet_forecast of the single
 * horizon t[k] under keys[k] ([S]; NULL: the rule above with the series' current observation index), from the same launch.  state_*
 * [S][d], the others [S], any may be NULL; the entries of a series that is inactive, has no cloud (CSSM_ESTATE) or fails
 * (CSSM_ENONFINITE) are not written, as its ll_out / ess_out entries are not; an active series whose time is refused, or whose model
 * lacks its scale (fc_rc_out[k] = CSSM_EINVAL_ARG), reads NaN and -1.  Null t / y / rc_out / fc_rc_out, an interval outside (0, 1] and a
 * null fleet are refused with CSSM_EINVAL_ARG before the fleet is looked at.  The device time is cssm_fleet_last_ms()[0]. */
int cssm_fleet_step_forecast(cssm_fleet* f, const uint8_t* active, const double* t, const double* y, const uint8_t* has_obs,
                             const uint64_t* keys, double interval, double* ll_out, int32_t* ess_out,
                             double* state_mean, double* state_lower, double* state_upper,
                             double* eta_mean, double* eta_lower, double* eta_upper,
                             double* obs_mean, double* obs_lower, double* obs_upper,
                             int32_t* obs_below, int32_t* obs_equal, int* rc_out, int* fc_rc_out);

/* cssm_pf_summary (getIntervals, model/ParticleFilter.scala:415-424) of every series at its own time: state_* [S * d], eta_* [S];
 * any may be NULL.  Order statistics exact, ranks and clamping as documented there, means plain fp64 sums.  A series without a
 * cloud reads NaN. */
int cssm_fleet_summary(cssm_fleet* f, double interval, double* state_mean, double* state_lower, double* state_upper,
                       double* eta_of_mean, double* eta_lower, double* eta_upper);
/* the cloud (SoA, d x N, as cssm_pf_get_particles) and the ancestors of series k; CSSM_ESTATE without a cloud */
int cssm_fleet_get_particles(cssm_fleet* f, uint32_t k, double* out_dN);
int cssm_fleet_get_ancestors(cssm_fleet* f, uint32_t k, uint32_t* out_N);
/* Forecasts of every series from its current cloud, all horizons of all series in ONE launch (one workgroup per series): the scan of
 * SimulateData.forecast + summariseForecast (model/Data.scala:196-231, model/ParticleFilter.scala:368-409).  Ragged as
 * cssm_fleet_ll_filter: series k owns the future times t[off[k] .. off[k+1]) (off[0] = 0, non-decreasing, S + 1 entries); a series
 * with no horizons is left alone (nothing is written for it, rc_out[k] = CSSM_OK).  keys[k] = the Philox key of series k's forecast
 * (the rule of thumb of cssm_pf_forecast: cssm_pf_run_key(seed_k, 2^63 | cssm_fleet_observation_index(f, k))).  Outputs are laid out
 * like t; with R = off[S]: state_* [R][d], eta_* / obs_* [R], the optional samples [R][d + 3][N] (rows: the d states, gamma, eta, obs);
 * any output may be NULL.
 *
 * Per series k the result is what cssm_pf_forecast(handle_k, t_k, H_k, keys[k], interval, ...) returns for a handle of its own --
 * cssm_pf_create(descs[k], N, seeds[k]) driven through the same calls: the source is the series' current cloud (what
 * cssm_fleet_summary reads), horizon h starts from horizon h - 1, the transition is the one an unweighted step with key keys[k] and
 * observation index h draws (CSSM_STREAM_STEP, paired streams, dt = 0 allowed), gamma and eta are taken at the series' own t[h] under
 * its own parameters, one observation draw on CSSM_STREAM_OBS with its own scale, ranks and clamping as documented at
 * cssm_pf_forecast.  Order statistics and samples are those bits; means are plain fp64 sums, so their order of summation may differ.
 *
 * The fleet is not touched: clouds, ancestors, clocks, observation indices, ll, ESS and keys stay as they were, and a following
 * cssm_fleet_step / cssm_fleet_summary returns what it would have without the forecast.
 *
 * rc_out[S] = the series' OWN status: CSSM_ESTATE for a series that has horizons but no cloud; CSSM_EINVAL_ARG for a series whose
 * times are not finite, start before its clock or decrease, and for a series whose model lacks the scale its observation needs
 * (cssm_last_error then carries the reference's exception for the first such series, although the call succeeds).  Such a series'
 * outputs read NaN, and every other series is bit for bit what it is without it.  The call itself fails only for errors that are not
 * one series' own: CSSM_EINVAL_ARG (null f / off / t / keys / rc_out, off[0] != 0 or off decreasing, interval outside (0, 1]),
 * CSSM_ESTATE when no series of the fleet has a cloud and R > 0, CSSM_ENOMEM, HIP failures.  With samples, the fleet runs in chunks
 * of series whose samples fit CSSM_OPT_FORECAST_CAP on the device (a series is never split). */
int cssm_fleet_forecast(cssm_fleet* f, const uint64_t* off, const double* t, const uint64_t* keys, double interval,
                        double* state_mean, double* state_lower, double* state_upper,
                        double* eta_mean, double* eta_lower, double* eta_upper,
                        double* obs_mean, double* obs_lower, double* obs_upper,
                        double* samples, int* rc_out);
/* SimulateData.simPompModel of every series in one launch per chunk: series k is simulated under its own parameters (those of
 * cssm_fleet_set_params), its own Philox key keys[k], from its own t0[k] over its own ragged times t[off[k] .. off[k + 1]) (off as for
 * cssm_fleet_forecast; T_k = 0 is allowed).  Every series gets its row at t0, so out (host) holds off[S] + S time indices of
 * (d + 3) x n_paths doubles each, series k's starting at index off[k] + k -- the indexing of cssm_fleet_filter's path_out.  n_paths is the
 * call's own (the fleet's N plays no part).  One thread per (series, pair of paths), flattened over the grid.
 * Series k's block is bit for bit cssm_simulate(descs[k], n_paths, keys[k], t0[k], t_k, T_k, ...).
 * The fleet is not touched: clouds, ancestors, clocks, keys, windows, ll and ESS stay as they were; no series needs a cloud.
 * rc_out[S] = the series' OWN status: CSSM_EINVAL_ARG for a t0 or times that are not finite, times before t0[k] or decreasing,
 * T_k >= 2^32 - 1, and for a model without the scale its observation needs (cssm_last_error names the first such series although the call
 * succeeds).  Such a series' rows read NaN; every other series is what it is without it.  The call itself fails, before any device call,
 * for a null f / t0 / off / keys / out / rc_out (t too when off[S] > 0), n_paths outside [1, 2^32 - 2^16], off[0] != 0 or off decreasing.
 * The fleet runs in chunks of series whose rows fit CSSM_OPT_FORECAST_CAP on the device; a single series beyond the cap runs in windows
 * of time indices with its states carried on the device.  The result does not depend on the cap. */
int cssm_fleet_simulate(cssm_fleet* f, uint64_t n_paths, const double* t0, const uint64_t* off, const double* t, const uint64_t* keys,
                        double* out, int* rc_out);
/* Device time (ms: upload, kernels, read-back) of the fleet's last cssm_fleet_simulate; CSSM_ESTATE before one. */
int cssm_fleet_simulate_last_ms(cssm_fleet* f, double* ms);
/* Posterior-predictive forecasts of every series in one launch: SimulateData.forecast(unparamModel, t, n)(posterior) + summariseForecast
 * (model/Data.scala:196-231) per series, each under its OWN joint posterior sample -- what S chains of cssm_fleet_pmmh_run leave.
 * Ragged posteriors: series k owns the pairs moff[k] .. moff[k+1]-1 (moff[0] = 0, non-decreasing, S + 1 entries; M_k = their number);
 * pair m is theta[m * n_theta ..] in flatten order and x[m * d ..], its state at t0[k].  off, t, keys, interval and the layout of every
 * output are cssm_fleet_forecast's.  pick (optional): [S][N] host indices, series k's each below M_k; pick_out (optional): [S][N].
 *
 * Per series k the result is bit for bit what cssm_pf_forecast_posterior(handle of N particles, desc, theta_k, n_theta, x_k, M_k, t0[k],
 * t_k, H_k, pick_k or NULL, keys[k], interval, ...) returns -- order statistics, samples and picks; means are plain fp64 sums, so their
 * order of summation may differ.  f(x, t) is that of series k's model (f has no parameters).  A series without horizons still gets its
 * pick_out row when M_k > 0; the pick_out row of a refused series, or of one with M_k = 0, reads 0.
 *
 * The fleet lends its device, stream, contract table, N, structure and scratch, as a handle does to cssm_pf_forecast_posterior: clouds,
 * ancestors, clocks, observation indices, ll, ESS, keys and parameters of every series stay as they were, and no series needs a cloud
 * (a fleet that was never initialised serves the call).
 *
 * rc_out[S] = the series' OWN status, CSSM_EINVAL_ARG for: horizons with M_k = 0; a theta row the model rejects or a non-finite theta
 * or x entry; pick >= M_k; a t0 or times that are not finite, times before t0[k] or decreasing; a descriptor without the scale its
 * observation needs (every series with M_k > 0, with or without horizons, as the single handle refuses it for any H).  Such a series' outputs read NaN, every other series is bit for bit what it is without it, the call succeeds and
 * cssm_last_error names the first such series and its row ("series k: theta row m: ...").  The call itself fails, before the fleet is
 * looked at, for: a null f / desc / moff / theta / x / t0 / off / t / keys / rc_out, moff[0] or off[0] != 0 or either decreasing, interval
 * outside (0, 1], n_theta not the descriptor's (CSSM_EINVAL_ARG); a descriptor of another structure than the fleet's, LGCP among them
 * (CSSM_EINVAL_DESC).  With samples, the fleet runs in chunks of series whose samples fit CSSM_OPT_FORECAST_CAP (a series is never
 * split); CSSM_OPT_FLEET_SELECT applies; the device time is cssm_fleet_last_ms()[2]. */
int cssm_fleet_forecast_posterior(cssm_fleet* f, const cssm_model_desc* desc,
                                  const uint64_t* moff, const double* theta, size_t n_theta, const double* x,
                                  const double* t0, const uint64_t* off, const double* t,
                                  const uint32_t* pick, const uint64_t* keys, double interval,
                                  double* state_mean, double* state_lower, double* state_upper,
                                  double* eta_mean, double* eta_lower, double* eta_upper,
                                  double* obs_mean, double* obs_lower, double* obs_upper,
                                  double* samples, uint32_t* pick_out, int* rc_out);
/* FilterInterpolate (model/ParticleFilter.scala:273-311, examples/Interpolate.scala:31-44) of every series: cssm_pf_interpolate on a
 * handle of its own, cssm_pf_create(descs[k], N, seeds[k]), per series -- in two launches for the whole fleet: a forward pass that keeps
 * every cloud and every weighted record's ancestors of a series ((T_k + 1) x N x (8 d + 4) bytes, the single handle's figure), one
 * workgroup per series, and a backward pass that composes the lineages surviving to the end of the series and summarises them per time
 * index, one workgroup per (series, row).  off / t / y / has_obs are ragged as for cssm_fleet_ll_filter (series k owns the records
 * off[k] .. off[k + 1] - 1, its t0 is its slice's smallest time); the outputs are laid out like cssm_fleet_filter's path_out: series k owns
 * the rows off[k] + k .. off[k + 1] + k (T_k + 1 rows, row 0 the initial cloud), state_* = [off[S] + S][d], eta_* = [off[S] + S]; any of
 * them may be null, ll_out[S] and rc_out[S] may not.  flags: 0 or CSSM_INTERP_REFERENCE_PAIRING, as for cssm_pf_interpolate.
 * ll_out[k] and every order statistic (state_lower / upper, eta_lower / upper) have the single handle's bits; the means are plain fp64
 * sums whose order of summation may differ, eta_of_mean = link(f(mean, time)) is formed on the host from the mean as there.
 *
 * The fleet is only LENT: its device, stream, contract table, N, structure, parameters and keys.  The clouds, ancestors, clocks,
 * observation indices and statuses of its series stay as they were -- a following cssm_fleet_step / _summary / _forecast returns what it
 * would have returned without this call, and a fleet that was never initialised serves it.  (The single handle borrows its own buffers
 * and must be re-initialised; the fleet's history lives in a slab of its own.)
 *
 * rc_out[S] = the series' OWN status: CSSM_EINVAL_ARG for a series without records (its single row and ll_out[k] read NaN),
 * CSSM_ENONFINITE when its weights were unusable at some observation (all its rows and ll_out[k] read NaN: the single handle returns no
 * summaries then either); every other series is bit for bit what it is without that one.  The call itself fails, before the fleet is
 * looked at, for a null off / ll_out / rc_out / t / y / f, off[0] != 0, interval outside (0, 1] or unknown flag bits, and for a
 * decreasing off (CSSM_EINVAL_ARG); CSSM_ENOMEM and HIP failures fail it too.  The fleet runs in chunks of series whose history fits
 * CSSM_OPT_INTERP_CAP (a series is never split; one larger than the cap runs alone, and CSSM_ENOMEM names it if it does not fit the
 * device): per chunk one upload, the two launches, one read-back. */
int cssm_fleet_interpolate(cssm_fleet* f, const uint64_t* off, const double* t, const double* y, const uint8_t* has_obs,
                           double interval, int flags, double* ll_out,
                           double* state_mean, double* state_lower, double* state_upper,
                           double* eta_of_mean, double* eta_lower, double* eta_upper, int* rc_out);
/* ms2[0] = device time of the forward launch, ms2[1] = of the lineage launch of the last cssm_fleet_interpolate, each summed over its
 * chunks (HIP events on the fleet's stream).  CSSM_ESTATE before the first interpolation.  The array holds TWO doubles. */
int cssm_fleet_interpolate_last_ms(cssm_fleet* f, double* ms2);
/* ---- EXTENSION (not a restatement of running reference code: the reference has no smoother beyond FilterInterpolate): forward filtering,
 * backward simulation (FFBSi; Godsill, Doucet and West 2004) of every series.  cssm_fleet_interpolate summarises time index s through the
 * lineages that survive to the end of the series; after a few dozen weighted records they pass through a handful of ancestors, and the
 * early rows are order statistics of one or two values.  cssm_fleet_smooth runs the same forward pass (the same history, chunks and
 * ll_out bits) and then draws n_traj trajectories BACKWARDS through the kept clouds: from its particle at index s + 1 a trajectory picks
 * its slot at index s among all N with probability proportional to the transition density, which is a diagonal Gaussian in closed form
 * for every transition of the library.  The arithmetic is part of the numerics contract (include/cssm_numerics.h, "backward
 * simulation"): IEEE operations and exact integer sums, one Philox uniform per (series key, trajectory, time index) under
 * CSSM_STREAM_BACK; a record with dt = 0 or a zero diffusion follows the genealogy.  Three launches per chunk of series: the forward
 * pass, k_fleet_backsim (blocks: series x groups of 64 trajectories) and the row summaries (one workgroup per (series, row)).
 *
 * off / t / y / has_obs, the output rows, ll_out, rc_out, the statuses, the chunks under CSSM_OPT_INTERP_CAP and what is refused before the
 * fleet is looked at are cssm_fleet_interpolate's; the fleet is only lent, and an open window is not touched.  Row s of series k
 * summarises the n_traj states the trajectories hold at time index s: the mean is their plain fp64 sum / n_traj, lower / upper are the
 * order statistics at the ranks cssm_pf_summary takes for n_traj values, exact.  1 <= n_traj <= CSSM_FLEET_MAX_N (else CSSM_EINVAL_ARG);
 * flags must be 0 -- CSSM_INTERP_REFERENCE_PAIRING is refused by name; an LGCP fleet is refused (its transition over an event is a chain
 * of sub-steps, not one Gaussian).  traj_out (may be NULL): [off[S] + S][n_traj], entry [row][m] the particle of slice `row` (an index
 * into the cloud that record proposed, < N) trajectory m passes through; the rows of a series whose rc_out is not 0 read 0xffffffff. */
int cssm_fleet_smooth(cssm_fleet* f, const uint64_t* off, const double* t, const double* y, const uint8_t* has_obs,
                      uint32_t n_traj, double interval, int flags, double* ll_out,
                      double* state_mean, double* state_lower, double* state_upper,
                      double* eta_of_mean, double* eta_lower, double* eta_upper,
                      uint32_t* traj_out, int* rc_out);
/* ms3 = device time of the forward launch, of the backward simulation and of the row summaries of the last cssm_fleet_smooth, each summed
 * over its chunks (HIP events on the fleet's stream).  CSSM_ESTATE before the first.  The array holds THREE doubles. */
int cssm_fleet_smooth_last_ms(cssm_fleet* f, double* ms3);
/* ---- EXTENSION (not a restatement of running reference code: the reference has no likelihood maximiser; examples/DetermineParameters.scala
 * assumes the starting value of its chains): maximum likelihood by iterated filtering -- IF2 of Ionides, Nguyen, Atchade, Stoev and King
 * (PNAS 2015), the `mif2` of the R package pomp.  S independent searches, one per series of the fleet and one workgroup each: every
 * particle carries its own parameter vector (the flattened STORED vector, cssm_desc_flatten order, n_theta slots), which random-walks
 * with a shrinking step before the initial draw and before every record and is resampled together with the state; after a few dozen
 * passes over the data the swarm sits at the maximum of the likelihood.  All n_iters iterations x T_k records of a search run inside
 * ONE launch (k_fleet_if2): transition coefficients and density constants are formed per particle on the device.  The arithmetic is
 * part of the numerics contract (include/cssm_numerics.h, "iterated filtering").
 *
 * The fleet is only LENT (device, stream, contract table, N, structure): clouds, clocks, keys, windows and parameters of its series stay
 * as they were, as cssm_fleet_smooth leaves them.  `desc` gives the structure (the fleet's, else CSSM_EINVAL_DESC) -- its parameter values
 * are not read.  Start: theta0[S][n_theta], one row per series that every particle starts from, or swarm0[S][n_theta][N] (wins when both
 * are given), the swarm_out of an earlier call.  The call runs iterations m = first_iter .. first_iter + n_iters - 1 of the search:
 * iteration m runs under cssm_pf_run_key(seeds[k], m + 1) and cools by cool_m = cooling_fraction_50^(m / 50) (cssm_fleet_if2_cooling),
 * so a search continued from swarm_out with first_iter = the iterations done so far is bit for bit the uninterrupted one.  rw_sd[n_theta] >= 0, finite:
 * the random-walk standard deviation per slot at m = 0; 0 keeps a slot's bits.  The slots of m0 and c0 are perturbed once per iteration,
 * before x0 is drawn (pomp's ivp), all others before x0 and before every record.  off / t / y / has_obs: the ragged data of
 * cssm_fleet_ll_filter.  iters_per_launch bounds the iterations one launch runs (0: all of them); the result does not depend on it.
 *
 * Outputs: theta_mean[S][n_iters][n_theta] (the swarm's mean per slot after each iteration of the call, a pairwise tree over the particle index),
 * ll[S][n_iters] (the perturbed filter's log-likelihood estimate, a diagnostic -- not the likelihood at the mean), rc_out[S]; optional
 * (may be NULL) swarm_out[S][n_theta][N] (the final swarm), and of the LAST iteration ll_t / ess_t (per record, off's layout),
 * x_out[S][d][N] (the cloud the last record proposed) and anc_out[S][N] (the ancestors that resampled it).  A record none of whose
 * particles has a usable weight ends that series' search: rc_out[k] = CSSM_ENONFINITE, its rows from the failing iteration on read NaN,
 * its swarm_out is the swarm that iteration started from, its last-iteration outputs read NaN / -1 / 0xffffffff; the others run on, bit
 * for bit what they are without it.  (A NaN log-weight of one particle is weight zero, not a failure.)  A series without records is
 * untouched: rc_out[k] = CSSM_OK, its rows read NaN.
 *
 * Refused before the fleet is looked at (CSSM_EINVAL_ARG unless said): null desc / rw_sd / seeds / off / theta_mean / ll / rc_out / t / y,
 * theta0 and swarm0 both null, off[0] != 0, a negative or non-finite rw_sd, n_iters outside [1, 1000000] or first_iter + n_iters beyond 2^31, cooling_fraction_50 outside
 * (0, 1], an invalid descriptor or the LGCP observation model (CSSM_EINVAL_DESC), n_theta other than the descriptor flattens to (at most
 * 81), an LGCP fleet (by name), a null fleet; then a decreasing off and another structure than the fleet's (CSSM_EINVAL_DESC). */
int cssm_fleet_if2(cssm_fleet* f, const cssm_model_desc* desc, const double* theta0, const double* swarm0, size_t n_theta,
                   const double* rw_sd, double cooling_fraction_50, uint32_t first_iter, uint32_t n_iters, uint32_t iters_per_launch,
                   const uint64_t* seeds, const uint64_t* off, const double* t, const double* y, const uint8_t* has_obs,
                   double* theta_mean, double* ll, double* swarm_out, double* ll_t, int32_t* ess_t, double* x_out,
                   uint32_t* anc_out, int* rc_out);
/* *ms = device time of the launches of the last cssm_fleet_if2 (HIP events on the fleet's stream); CSSM_ESTATE before the first. */
int cssm_fleet_if2_last_ms(cssm_fleet* f, double* ms);
/* No device: cool[q] = cooling_fraction_50^((first_iter + q) / 50), q < n_iters, the array the call cools by (whoever restates a search
 * takes it from here, not from another pow). */
int cssm_fleet_if2_cooling(double cooling_fraction_50, uint32_t first_iter, uint32_t n_iters, double* cool);
/* Diagnostic, no device: where the flattened vector of `desc` holds what each latent component reads.  out = d, n_theta, obs_kind,
 * obs_df, the scale's slot (-1: none); per component 10 integers: sde_kind, leaf, index in the leaf, f_kind, period, then the slots of
 * m0, c0, mu, phi, sigma (-1: the SDE has no such field); then n_theta flags: 1 = the slot only feeds the initial draw.  *count = the
 * integers that is (5 + 10 d + n_theta); out may be NULL to ask for it. */
int cssm_fleet_if2_layout(const cssm_model_desc* desc, int32_t* out, size_t cap, size_t* count);

/* ---- whole PMMH chains on the device (model/PMMH.scala:32,68-81 with the reference's own prior argument; Parameters.perturbMvn,
 * model/Parameters.scala:111-123).  S chains, a chain per series and ONE WORKGROUP PER CHAIN: every iteration and every record of a
 * chain runs inside k_fleet_pmmh, the record built in the block from the chain's own parameter row, so the host does nothing between
 * iterations.  The arithmetic is the contract's (include/cssm_numerics.h, "PMMH chains on the device").
 *
 * Chain k starts at theta0[k * n_theta ..] (cssm_desc_flatten order of `desc`, which gives the STRUCTURE only), runs under seeds[k] and
 * sees series k's slice of the data (off / t / y / has_obs as cssm_fleet_ll_filter).  chol: the lower-triangular factor L of the
 * proposal's covariance, row-major [n_theta][n_theta] -- one for all chains (chol_per_chain = 0) or one per chain (!= 0, [S][..][..]);
 * entries above the diagonal must be 0.0, a row of zeros fixes its slot, L = sqrt(delta) I is cssm_fleet_pmmh_run's proposal.  priors:
 * [n_theta] cssm_prior, one per slot, on the STORED value; NULL = all flat (declared const void*, as every fleet call takes scalar
 * pointers and handles only; a const cssm_prior* converts implicitly).  ll0 / state0: the chain's current log-likelihood and sampled state ([S], [S][d]);
 * NULL = -1e99 / zeros, a fresh chain (PMMH.scala:121).  Iteration q of the call is iteration first_iter + q of the chain: a chain
 * continued with first_iter = the iterations done, theta0 / ll0 / state0 = its last row is the uninterrupted chain bit for bit (accepted
 * restarts at 0 per call).  iters_per_launch (0 = all) bounds a launch without changing a bit.  Outputs chain-major as
 * cssm_fleet_pmmh_run: ll[k * n_iters + q], theta[(k * n_iters + q) * n_theta + j], accepted[..], last_state[(k * n_iters + q) * d + c].
 * diag_out (may be NULL; [S][2]): proposals rejected unfiltered (outside the prior's support) | proposals whose filter had no usable
 * weight.  With all priors flat and a diagonal L the rows are cssm_fleet_pmmh_run's bit for bit.
 * Unlike cssm_fleet_pmmh_run, which ends the whole run on a proposal the descriptor path refuses, a proposal that is not filtered is a
 * REJECTION here and the chain goes on; and a series without records is not refused: it is untouched, its rows read NaN (accepted -1),
 * rc_out[k] = CSSM_EINVAL_ARG.  Every other series has rc_out[k] = CSSM_OK.
 * The fleet is only LENT (as to cssm_fleet_if2): device, stream, contract table, N and structure; clouds, clocks, keys, windows and
 * parameters stay as they were, the call keeps buffers of its own.
 * Refused before the fleet is looked at (CSSM_EINVAL_ARG unless said): null desc / theta0 / chol / seeds / off / t / y or outputs (ll,
 * theta, accepted, last_state, rc_out); off[0] != 0; an LGCP descriptor (CSSM_EINVAL_DESC); n_theta other than the descriptor flattens to
 * (at most CSSM_IF2_MAX_THETA = 81); a chol entry that is not finite or lies above the diagonal and is not 0.0; a NORMAL prior whose b is
 * not finite and positive or whose a is not finite, a UNIFORM prior with a > b or a NaN bound, an unknown kind; n_iters outside
 * [1, 1000000]; first_iter + n_iters > 2^31; an LGCP fleet.  After the fleet is looked at (it says how many chains there are): off
 * decreasing, a descriptor of another structure than the fleet's (CSSM_EINVAL_DESC), a theta0 row whose prior is -inf or NaN (outside
 * the support), a chol_per_chain factor beyond the first that fails the test above.
 * Not served (cssm_pmmh_run / _run_batched / _run_speculative keep the flat prior and the isotropic proposal): single handles and
 * batches, covariance updates inside the kernel.  LGCP fleets and LGCP descriptors are refused here by name: cssm_fleet_pmmh_chains_lgcp
 * (below) runs their chains. */
#define CSSM_PRIOR_FLAT    0   /* contributes nothing */
#define CSSM_PRIOR_NORMAL  1   /* on the STORED value: -(z*z)/2.0, z = (theta - a) / b, b > 0 (constants dropped: only differences decide) */
#define CSSM_PRIOR_UNIFORM 2   /* 0.0 if a <= theta <= b, else -inf */
typedef struct { int32_t kind; int32_t pad_; double a, b; } cssm_prior;
int cssm_fleet_pmmh_chains(cssm_fleet* f, const cssm_model_desc* desc, const double* theta0, size_t n_theta,
                           const double* chol, int chol_per_chain, const void* priors, const double* ll0, const double* state0,
                           uint32_t first_iter, uint32_t n_iters, uint32_t iters_per_launch,
                           const uint64_t* seeds, const uint64_t* off, const double* t, const double* y, const uint8_t* has_obs,
                           double* ll, double* theta, int32_t* accepted, double* last_state, uint32_t* diag_out, int* rc_out);
/* *ms = device time of the launches of the last cssm_fleet_pmmh_chains (HIP events on the fleet's stream); CSSM_ESTATE before the first. */
int cssm_fleet_pmmh_chains_last_ms(cssm_fleet* f, double* ms);
/* ---- whole PMMH chains for LGCP fleets: cssm_fleet_pmmh_chains over FilterLgcp (model/ParticleFilter.scala:169-227), asked for by name
 * as cssm_fleet_create_lgcp is.  One workgroup per chain: every iteration and every event of a chain runs inside k_fleet_pmmh_lgcp; the
 * arithmetic is the contract's (include/cssm_numerics.h, "PMMH chains on the device: LGCP").  With all priors flat and L = sqrt(delta) I
 * chain k is cssm_pmmh_run on an LGCP handle of N particles under seeds[k], bit for bit.
 *
 * The semantics are cssm_fleet_pmmh_chains's word for word -- chol (one for all chains or one per chain), priors, ll0 / state0,
 * first_iter, iters_per_launch (0 = all; never changes a bit), chain-major outputs, diag_out[S][2], a series without events untouched
 * (NaN rows, accepted -1, rc_out[k] = CSSM_EINVAL_ARG) -- with these differences: f is an LGCP fleet; every record is an event, so there
 * is no y and no has_obs; desc is an LGCP descriptor whose lgcp_precision is part of the structure and must be the fleet's.  A series'
 * first increment starts at its smallest time, as in cssm_fleet_filter on a fresh series.
 * The fleet is only LENT: clouds, ancestors, ll / ess, clocks, observation indices, keys, parameters and every series' predicted level
 * are afterwards what they were; the call keeps buffers of its own, among them the per-event records (24 + 8 d bytes: what does not
 * depend on the parameters) and, where f depends on time, the sub-step table of all chains (at most 1 GiB, else CSSM_ENOMEM), both
 * uploaded once per call.
 * Refused before the fleet is looked at (CSSM_EINVAL_ARG unless said): null desc / theta0 / chol / seeds / off / t or outputs (ll, theta,
 * accepted, last_state, rc_out); off[0] != 0; a descriptor that is not LGCP (CSSM_EINVAL_DESC, naming cssm_fleet_pmmh_chains); n_theta
 * other than the descriptor flattens to; a bad chol entry; a bad prior; n_iters outside [1, 1000000]; first_iter + n_iters > 2^31; a null
 * fleet.  Then: a fleet that cssm_fleet_create_lgcp did not make (naming cssm_fleet_pmmh_chains); off decreasing; a descriptor of
 * another structure or precision than the fleet's (CSSM_EINVAL_DESC); a theta0 row outside the prior's support; a chol_per_chain
 * factor beyond the first that fails the test.
 * Not served: cssm_fleet_pmmh_run and cssm_fleet_if2 for LGCP fleets, the C++ mirror and JNI, other resamplers than systematic,
 * covariance updates inside the kernel. */
int cssm_fleet_pmmh_chains_lgcp(cssm_fleet* f, const cssm_model_desc* desc, const double* theta0, size_t n_theta,
                                const double* chol, int chol_per_chain, const void* priors, const double* ll0, const double* state0,
                                uint32_t first_iter, uint32_t n_iters, uint32_t iters_per_launch,
                                const uint64_t* seeds, const uint64_t* off, const double* t,
                                double* ll, double* theta, int32_t* accepted, double* last_state, uint32_t* diag_out, int* rc_out);
/* *ms = device time of the launches of the last cssm_fleet_pmmh_chains_lgcp (HIP events on the fleet's stream); CSSM_ESTATE before the first. */
int cssm_fleet_pmmh_chains_lgcp_last_ms(cssm_fleet* f, double* ms);
/* ---- fixed-lag interpolation of a live fleet (FilterInterpolate as the stream it is: ParticleFilter.interpolate, model/
 * ParticleFilter.scala:281-310 -- one stepInterpolate per observation, every element carrying the paths that survive to that moment;
 * examples/Interpolate.scala: once data resumes behind a gap, the surviving lineages fill it).
 *
 * cssm_fleet_window(f, slices): the fleet remembers, per series, its `slices` most recent clouds and ancestor arrays on the device --
 * S x slices x N x (8 d + 4) bytes (459 MB at S = 1024, N = 1000, d = 3, slices = 16).  slices >= 2 allocates and sets every series'
 * depth to 0 (re-opening, with the same size or another, restarts every window); 0 frees; 1 is CSSM_EINVAL_ARG.  An allocation that
 * does not fit is CSSM_ENOMEM naming the bytes, and the fleet goes on without a window.
 * cssm_fleet_window_depth(f, k): the records remembered behind series k's base slice, 0 .. slices - 1 (the base slice is not counted; a
 * full ring overwrites its oldest slice and the depth stays slices - 1); 0 for a null fleet, k >= S or no window.
 *
 * cssm_fleet_step_interpolate: cssm_fleet_step -- active / t / y / has_obs / ll_out / ess_out / rc_out are its arguments, bits and
 * statuses, and the cloud, ancestors, clock and observation index it leaves are the ones cssm_fleet_step leaves -- which also writes
 * every cloud it moved and the ancestors that resampled it into the series' window (one launch), and, for the series that ask, a second
 * launch: the summaries of the last lag + 1 time indices through the lineages that survive to the cloud just written, one workgroup per
 * (series, row).
 *   lag: [S], or NULL = max_lag for every series.  CSSM_FLEET_NO_ROWS: the series is stepped and remembered but not summarised --
 *   rows_out[k] = 0, nothing of its rows is written, no block of the second launch runs for it (a call in which no series asks is one
 *   launch).  Any other lag[k] above max_lag fails the call (CSSM_EINVAL_ARG naming k).
 *   Outputs: state_* = [S][max_lag + 1][d], eta_* = [S][max_lag + 1], rows_out = [S]; any may be NULL.  For a series stepped through
 *   records 0 .. m by this call only, its window open since before record 0, row j (0 <= j <= min(lag_k, depth_k)) is bit for bit row
 *   m + 1 - j of cssm_fleet_interpolate over its records 0 .. m (flags 0, the same t0, parameters and key): j = 0 is the cloud just
 *   written through the ancestors that resampled it, the order statistics are exact, the means are k_fleet_lineage's sums in its order,
 *   eta_of_mean is formed on the host from the mean.  Rows min(lag_k, depth_k) < j <= max_lag read NaN; rows_out[k] = min(lag_k,
 *   depth_k) + 1.  The bounded window changes no row it still returns: the lineages are only ever composed from the newest index back.
 *   For a series that is inactive, has no cloud (CSSM_ESTATE) or fails (CSSM_ENONFINITE) no entry is written, as for ll / ess; a failed
 *   series loses its window.
 *   Continuity: a series' window is continuous only across consecutive cssm_fleet_step_interpolate calls that stepped it.  Every other
 *   call that writes its cloud, key or parameters (cssm_fleet_init, _init_from, _step, _step_intervals, _step_forecast, _ll_filter, _ll_filter_more, _filter,
 *   _filter_intervals, _filter_intervals_more, _filter_forecasts, _pmmh_run, _reseed, _set_params) sets its depth to 0, and the next cssm_fleet_step_interpolate
 *   first records the cloud the series holds then (what cssm_fleet_get_particles returns, identity ancestors) as the base slice at the
 *   series' clock: the rows never reach behind it, and from it on they are the prefix interpolation's.  Calls that only read
 *   (cssm_fleet_summary, the forecasts, cssm_fleet_interpolate, cssm_fleet_get_*) leave the windows alone, and cssm_fleet_interpolate
 *   does not touch them.
 *   CSSM_INTERP_REFERENCE_PAIRING is not offered: it pairs output row k with time index T - k, which has no meaning in a window whose
 *   T moves with every call.
 *   Errors: null t / y / rc_out, an interval outside (0, 1], a bad lag and a null fleet are refused with CSSM_EINVAL_ARG before the fleet
 *   is looked at; a fleet without a window is CSSM_ESTATE naming cssm_fleet_window; then as cssm_fleet_step.  The device time of the
 *   whole call is cssm_fleet_last_ms()[0].
 * cssm_fleet_step_interpolate_last_ms: ms2[0] = device time of the forward launch, ms2[1] = of the lineage launch (0 when no series
 * asked for rows) of the last cssm_fleet_step_interpolate; CSSM_ESTATE before the first.  The array holds TWO doubles. */
#define CSSM_FLEET_NO_ROWS 0xffffffffu
int cssm_fleet_window(cssm_fleet* f, uint32_t slices);
uint32_t cssm_fleet_window_depth(const cssm_fleet* f, uint32_t k);
int cssm_fleet_step_interpolate(cssm_fleet* f, const uint8_t* active, const double* t, const double* y, const uint8_t* has_obs,
                                const uint32_t* lag, uint32_t max_lag, double interval,
                                double* ll_out, int32_t* ess_out, uint32_t* rows_out,
                                double* state_mean, double* state_lower, double* state_upper,
                                double* eta_of_mean, double* eta_lower, double* eta_upper, int* rc_out);
int cssm_fleet_step_interpolate_last_ms(cssm_fleet* f, double* ms2);
/* Observations series k's current cloud has seen (the Philox counter word of its next step); 0 for a null fleet or k >= S, the
 * convention of cssm_pf_observation_index. */
uint64_t cssm_fleet_observation_index(const cssm_fleet* f, uint32_t k);
/* ms3[0] = device time of the last ll_filter / filter / init / step call (upload, launch, read-back), ms3[1] = of the last summary, ms3[2] =
 * of the last forecast (cssm_fleet_forecast or cssm_fleet_forecast_posterior); HIP events on the fleet's stream, < 0 while there was none.  The array holds THREE doubles. */
int cssm_fleet_last_ms(cssm_fleet* f, double* ms3);
/* Diagnostic, no device: the compact per-observation record the fleet uploads for (t_prev, t, y, has_obs, step) under `desc`,
 * a cloud of n_particles and Philox key `seed` -- 80 + 40 d bytes: y, c[4], cdf, u, dt, ref (doubles), has_obs (i32), step (u32),
 * then d x 4 transition coefficients and d f coefficients, each the value cssm_pf_step's record holds. */
int cssm_fleet_pack_record(const cssm_model_desc* desc, uint64_t n_particles, uint64_t seed, double t_prev, double t, double y,
                           int has_obs, uint32_t step, unsigned char* out, size_t cap, size_t* bytes);
/* Diagnostic, no device: the compact record an LGCP fleet uploads for the event at t behind t_prev under `desc` (CSSM_OBS_LGCP, else
 * CSSM_EINVAL_DESC) -- 32 + 40 d bytes: u, dt = 10^-precision (doubles), n_sub = ceil((t - t_prev) / dt) (i32), step, fsub_off, pick
 * (u32), then d x 4 transition coefficients over dt and d f coefficients at t -- and the rows of the sub-step table it brings:
 * fsub_count = n_sub x d coefficients of f at the sub-step times where f depends on time (a seasonal leaf), else 0; fsub_off = 0.
 * fsub_out may be NULL when nothing is brought; a table beyond fsub_cap is CSSM_EINVAL_ARG (fsub_count says what it needs). */
int cssm_fleet_pack_record_lgcp(const cssm_model_desc* desc, uint64_t n_particles, uint64_t seed, double t_prev, double t,
                                uint32_t step, unsigned char* out, size_t cap, size_t* bytes,
                                double* fsub_out, size_t fsub_cap, size_t* fsub_count);
/* Diagnostic, no device: the record cssm_fleet_pmmh_chains_lgcp uploads for the event at t behind t_prev under `desc` (CSSM_OBS_LGCP,
 * else CSSM_EINVAL_DESC) -- the part of the record above that does not depend on the parameters or the key, 24 + 8 d bytes: dt =
 * 10^-precision (double; 0 where n_sub == 0), n_sub (i32), step, fsub_off, a zero word (u32), then the d f coefficients at t -- and the
 * rows of the sub-step table it brings, as above. */
int cssm_fleet_pmmh_lgcp_pack_record(const cssm_model_desc* desc, double t_prev, double t, uint32_t step,
                                     unsigned char* out, size_t cap, size_t* bytes,
                                     double* fsub_out, size_t fsub_cap, size_t* fsub_count);

/* ---- errors / build info ------------------------------------------------------------------ */
const char* cssm_last_error(void);
const char* cssm_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CSSM_PF_H */
