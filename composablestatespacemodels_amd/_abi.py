"""ctypes view of include/cssm_pf.h and the loader of libcssm_pf.so.

The shared library is the product: hand-written HIP kernels for gfx950 behind a C ABI.  There is
no CPU fallback -- if the library has not been built (``python -c 'import __graft_entry__ as g;
g.build()'``) every entry point of this package raises.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CSSM_PF_LIB") or os.path.join(HERE, "csrc", "libcssm_pf.so")   # (CSSM_PF_LIB: an experiment build, tools/)

# ---- constants (include/cssm_pf.h) ---------------------------------------------------------
CSSM_OK = 0
CSSM_EINVAL_DESC = -1
CSSM_EHIP = -2
CSSM_ESHARD = -3
CSSM_ENOMEM = -4
CSSM_ENONFINITE = -5
CSSM_EINVAL_ARG = -6
CSSM_ESTATE = -7

SDE_BROWNIAN, SDE_GEN_BROWNIAN, SDE_OU, SDE_EULER_AFFINE = 0, 1, 2, 3
F_FIRST, F_SEASONAL = 0, 1
OBS_POISSON, OBS_GAUSSIAN, OBS_LGCP = 0, 1, 2
OBS_NEGBIN, OBS_ZIP, OBS_BERNOULLI, OBS_STUDENT_T, OBS_BETA = 3, 4, 5, 6, 7
MAX_DIM = 16
MAX_LEAVES = 16
FLEET_MAX_N = 4096   # CSSM_FLEET_MAX_N
CSSM_OPT_INTERP_CAP = 13
CSSM_OPT_SMOOTH_STAGING = 14   # cssm_fleet_smooth: 0 = the gathered cloud in LDS where it fits, 1 = never (through L2)
CSSM_OPT_SMOOTH_TILE = 15      # cssm_pf_smooth: the slots a block of the backward kernels stages (0 = SMOOTH_TILE; a multiple of 64)
SMOOTH_TILE = 512              # CSSM_SMOOTH_TILE
CSSM_INTERP_REFERENCE_PAIRING = 1
CSSM_FLEET_NO_ROWS = 0xFFFFFFFF
CSSM_PF_NO_ROWS = 0xFFFFFFFF      # cssm_pf_step_interpolate: step and remember, no rows
CSSM_FLEET_COPY_KEEP = -1         # cssm_fleet_copy_series, a map entry: leave the series exactly as it is
CSSM_FLEET_COPY_KEYS = 1          # ... flags: the Philox key travels too
CSSM_OPT_FORECAST_CAP = 11
CSSM_SIM_STEP_ROW0 = 0xFFFFFFFF   # include/cssm_obs_draws.h: the step of the observation drawn at t0
CSSM_LGCP_SIM_KEEP_GRID = 1       # cssm_simulate_lgcp: download the grid rows too
CSSM_STREAM_THIN = 10             # include/cssm_obs_draws.h: the candidates of simLGCP's thinning
CSSM_STREAM_IF2 = 12              # include/cssm_numerics.h: the perturbation normals of iterated filtering
IF2_MAX_THETA = 81                # CSSM_IF2_MAX_THETA
IF2_TILE = 1024                   # CSSM_IF2_TILE: the particles a block of cssm_pf_if2's tile launches owns
CSSM_PRIOR_FLAT, CSSM_PRIOR_NORMAL, CSSM_PRIOR_UNIFORM = 0, 1, 2   # cssm_prior.kind
CSSM_FN_EXP_LE0, CSSM_FN_LGAMMA, CSSM_FN_LGAMMA_KP1 = 8, 9, 10   # cssm_contract_eval: the contract functions evaluated per lane
CSSM_LGCP_PATH_OK, CSSM_LGCP_PATH_NONFINITE, CSSM_LGCP_PATH_TOO_MANY = 0, 1, 2   # a path's status

_dp = C.POINTER(C.c_double)


class LeafDesc(C.Structure):
    _fields_ = [
        ("sde_kind", C.c_int32), ("dim", C.c_int32), ("f_kind", C.c_int32), ("period", C.c_int32),
        ("harmonics", C.c_int32), ("has_scale", C.c_int32), ("scale", C.c_double),
        ("n_m0", C.c_int32), ("n_c0", C.c_int32), ("n_mu", C.c_int32), ("n_phi", C.c_int32),
        ("n_sigma", C.c_int32), ("reserved", C.c_int32),
        ("m0", _dp), ("c0", _dp), ("mu", _dp), ("phi", _dp), ("sigma", _dp),
    ]


class ModelDesc(C.Structure):
    _fields_ = [
        ("n_leaves", C.c_int32), ("obs_kind", C.c_int32), ("lgcp_precision", C.c_int32),
        ("obs_df", C.c_int32), ("leaves", C.POINTER(LeafDesc)),
    ]


class Prior(C.Structure):
    """cssm_prior: one slot's prior on the STORED value (cssm_fleet_pmmh_chains)."""
    _fields_ = [("kind", C.c_int32), ("pad_", C.c_int32), ("a", C.c_double), ("b", C.c_double)]


class PeerHandle(C.Structure):
    """cssm_peer_handle: what a rank hands the others so that they can map its receive windows (peer-written exchange)."""
    _fields_ = [("ipc", C.c_char * 64), ("pid", C.c_uint64), ("local_ptr", C.c_uint64), ("bytes", C.c_uint64),
                ("device", C.c_int32), ("has_ipc", C.c_int32)]


class CssmError(RuntimeError):
    """Raised for a non-zero status of a cssm_* call (the reference throws from stepFilter)."""

    def __init__(self, code: int, msg: str):
        super().__init__(f"cssm error {code}: {msg}")
        self.code = code


# Every symbol include/cssm_pf.h declares: (name, restype, argtypes)
_u64p = C.POINTER(C.c_uint64)
_i64p = C.POINTER(C.c_int64)
_i32p = C.POINTER(C.c_int32)
_u32p = C.POINTER(C.c_uint32)
_u8p = C.POINTER(C.c_uint8)
_descp = C.POINTER(ModelDesc)
_h = C.c_void_p

SYMBOLS = [
    ("cssm_pf_create", C.c_int, [_descp, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(_h)]),
    ("cssm_pf_create_shard", C.c_int, [_descp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p, C.POINTER(_h)]),
    ("cssm_pf_destroy", None, [_h]),
    ("cssm_pf_set_params", C.c_int, [_h, _descp]),
    ("cssm_pf_reseed", C.c_int, [_h, C.c_uint64]),
    ("cssm_pf_run_key", C.c_uint64, [C.c_uint64, C.c_uint64]),
    ("cssm_pf_get_weights", C.c_int, [_h, _dp, _dp]),
    ("cssm_pf_init", C.c_int, [_h, C.c_double]),
    ("cssm_pf_init_from", C.c_int, [_h, C.c_double, _dp]),
    ("cssm_pf_step", C.c_int, [_h, C.c_double, C.c_double, C.c_int, _dp, _i32p]),
    ("cssm_pf_propagate", C.c_int, [_h, C.c_double, C.c_double, C.c_int]),
    ("cssm_pf_adopt", C.c_int, [_h, _dp, C.c_double, C.c_int32]),
    ("cssm_pf_ll_filter", C.c_int, [_h, _dp, _dp, _u8p, C.c_size_t, _dp, _dp, _i32p]),
    ("cssm_pf_ll_filter_more", C.c_int, [_h, _dp, _dp, _u8p, C.c_size_t, _dp, _dp, _i32p]),
    ("cssm_pf_filter", C.c_int, [_h, _dp, _dp, _u8p, C.c_size_t, _dp, _dp, _i32p, _dp]),
    ("cssm_pf_last_loop_ms", C.c_int, [_h, C.POINTER(C.c_float)]),
    ("cssm_pf_last_device_us", C.c_int, [_h, _dp]),
    ("cssm_pf_stream_idle", C.c_int, [_h]),
    ("cssm_pf_set_option", C.c_int, [_h, C.c_int, C.c_int]),
    ("cssm_rtc_info", C.c_int, [_u64p]),
    ("cssm_pf_profile", C.c_int, [_h, C.c_int]),
    ("cssm_pf_profile_read", C.c_int, [_h, _dp, _u64p]),
    ("cssm_pf_num_particles", C.c_uint64, [_h]),
    ("cssm_pf_dim", C.c_int32, [_h]),
    ("cssm_pf_get_particles", C.c_int, [_h, _dp]),
    ("cssm_pf_get_ancestors", C.c_int, [_h, _u32p]),
    ("cssm_pf_get_logw", C.c_int, [_h, _dp]),
    ("cssm_pf_get_proposed", C.c_int, [_h, _dp]),
    ("cssm_pf_summary", C.c_int, [_h, C.c_double, _dp, _dp, _dp, _dp, _dp, _dp]),
    ("cssm_pf_filter_intervals", C.c_int, [_h, _dp, _dp, _u8p, C.c_size_t, C.c_double, _dp, _dp, _i32p, _dp, _dp, _dp, _dp, _dp, _dp]),
    ("cssm_pf_filter_intervals_more", C.c_int, [_h, _dp, _dp, _u8p, C.c_size_t, C.c_double, _dp, _dp, _i32p, _dp, _dp, _dp, _dp, _dp, _dp]),
    ("cssm_pf_step_intervals", C.c_int, [_h, C.c_double, C.c_double, C.c_int, C.c_double, _dp, _i32p, _dp, _dp, _dp, _dp, _dp, _dp]),
    ("cssm_pf_intervals_last_ms", C.c_int, [_h, _dp]),
    ("cssm_pf_filter_forecasts", C.c_int, [_h, _dp, _dp, _u8p, C.c_size_t, _u64p, C.c_double, _dp, _dp, _i32p, _dp, _dp, _dp, _dp, _dp, _dp,
                                           _dp, _dp, _dp, _i32p, _i32p]),
    ("cssm_pf_filter_forecasts_more", C.c_int, [_h, _dp, _dp, _u8p, C.c_size_t, _u64p, C.c_double, _dp, _dp, _i32p, _dp, _dp, _dp, _dp, _dp, _dp,
                                                _dp, _dp, _dp, _i32p, _i32p]),
    ("cssm_pf_step_forecast", C.c_int, [_h, C.c_double, C.c_double, C.c_int, C.c_uint64, C.c_int, C.c_double, _dp, _i32p, _dp, _dp, _dp, _dp,
                                        _dp, _dp, _dp, _dp, _dp, _i32p, _i32p]),
    ("cssm_pf_forecasts_last_ms", C.c_int, [_h, _dp]),
    ("cssm_pf_forecast", C.c_int, [_h, _dp, C.c_size_t, C.c_uint64, C.c_double, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    ("cssm_pf_forecast_posterior", C.c_int, [_h, _descp, _dp, C.c_size_t, _dp, C.c_size_t, C.c_double, _dp, C.c_size_t, _u32p, C.c_uint64,
                                             C.c_double, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _u32p]),
    ("cssm_pf_forecast_last_ms", C.c_int, [_h, _dp]),
    ("cssm_pf_observation_index", C.c_uint64, [_h]),
    ("cssm_obs_draw", C.c_int, [C.c_int, _dp, C.c_size_t, C.c_int, C.c_double, C.c_int, C.c_uint64, C.c_uint32, _dp, C.c_int]),
    ("cssm_simulate", C.c_int, [_descp, C.c_uint64, C.c_uint64, C.c_double, _dp, C.c_size_t, C.c_size_t, C.c_int, _dp]),
    ("cssm_simulate_from", C.c_int, [_descp, C.c_uint64, C.c_uint64, _dp, C.c_uint32, C.c_double, _dp, C.c_size_t, C.c_size_t, C.c_int, _dp]),
    ("cssm_simulate_last_ms", C.c_int, [_dp]),
    ("cssm_simulate_lgcp", C.c_int, [_descp, C.c_uint64, C.c_uint64, C.c_double, C.c_double, C.c_int, C.c_int, C.c_size_t, C.c_int, C.POINTER(_h)]),
    ("cssm_lgcp_sim_shape", C.c_int, [_h, C.POINTER(C.c_int), _u64p, _u64p, _u64p]),
    ("cssm_lgcp_sim_grid_times", C.c_int, [_h, _dp]),
    ("cssm_lgcp_sim_grid", C.c_int, [_h, _dp]),
    ("cssm_lgcp_sim_paths", C.c_int, [_h, _u64p, _dp, _u32p, _i32p]),
    ("cssm_lgcp_sim_events", C.c_int, [_h, _dp, _u32p, _dp]),
    ("cssm_lgcp_sim_destroy", None, [_h]),
    ("cssm_simulate_lgcp_last_ms", C.c_int, [_dp]),
    ("cssm_pf_interpolate", C.c_int, [_h, _dp, _dp, _u8p, C.c_size_t, C.c_double, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    ("cssm_pf_smooth", C.c_int, [_h, _dp, _dp, _u8p, C.c_size_t, C.c_uint32, C.c_double, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _u32p]),
    ("cssm_pf_smooth_last_ms", C.c_int, [_h, _dp]),
    ("cssm_pf_if2", C.c_int, [_h, _dp, _dp, C.c_size_t, _dp, C.c_double, C.c_uint32, C.c_uint32, C.c_uint64, _dp, _dp, _u8p, C.c_size_t,
                              _dp, _dp, _dp, _dp, _i32p, _dp, _u32p]),
    ("cssm_pf_if2_last_ms", C.c_int, [_h, _dp]),
    ("cssm_pf_window", C.c_int, [_h, C.c_uint32]),
    ("cssm_pf_window_depth", C.c_uint32, [_h]),
    ("cssm_pf_step_interpolate", C.c_int, [_h, C.c_double, C.c_double, C.c_int, C.c_uint32, C.c_double, _dp, _i32p, _u32p, _dp, _dp, _dp, _dp, _dp, _dp]),
    ("cssm_pf_step_interpolate_last_ms", C.c_int, [_h, _dp]),
    ("cssm_resample_systematic", C.c_int, [_dp, C.c_size_t, C.c_double, _u32p, C.c_int]),
    ("cssm_resample", C.c_int, [C.c_int, _dp, C.c_size_t, C.c_double, C.c_uint64, C.c_uint32, _u32p, C.c_int]),
    ("cssm_resample_residual", C.c_int, [_dp, C.c_size_t, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint32), C.c_int]),
    ("cssm_pf_shard_init", C.c_int, [_h, C.c_double]),
    ("cssm_pf_shard_propagate", C.c_int, [_h, C.c_double, C.c_double, C.c_int, C.c_void_p]),
    ("cssm_pf_shard_sums", C.c_int, [_h, C.c_void_p, C.c_int, C.c_void_p]),
    ("cssm_pf_shard_offspring", C.c_int, [_h, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("cssm_pf_shard_begin", C.c_int, [_h, _dp, _dp, _u8p, C.c_size_t]),
    ("cssm_pf_shard_continue", C.c_int, [_h, _dp, _dp, _u8p, C.c_size_t]),
    ("cssm_pf_shard_propagate_at", C.c_int, [_h, C.c_size_t, C.c_void_p]),
    ("cssm_pf_shard_wait_stats", C.c_int, [_h, _u64p]),
    ("cssm_pf_shard_status", C.c_int, [_h, _dp, _i32p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_size_t]),
    ("cssm_pf_shard_want_path", C.c_int, [_h, C.c_int]),
    ("cssm_pf_shard_get_path", C.c_int, [_h, _dp, C.c_size_t]),
    ("cssm_model_structure", C.c_int, [_descp, C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]),
    ("cssm_pf_shard_summary_begin", C.c_int, [_h, C.c_double, C.c_void_p, C.c_void_p]),
    ("cssm_pf_shard_summary_hist", C.c_int, [_h, C.c_int, C.c_void_p]),
    ("cssm_pf_shard_summary_pick", C.c_int, [_h, C.c_int, C.c_void_p]),
    ("cssm_pf_shard_summary_finish", C.c_int, [_h, C.c_void_p, _dp, _dp, _dp, _dp, _dp, _dp]),
    ("cssm_pf_shard_pack", C.c_int, [_h, C.c_int, _i64p, _i64p, C.c_int, C.c_void_p]),
    ("cssm_pf_shard_adopt", C.c_int, [_h, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64]),
    ("cssm_pf_shard_result", C.c_int, [_h, _dp, _i32p]),
    ("cssm_rccl_available", C.c_int, []),
    ("cssm_rccl_library", C.c_char_p, []),
    ("cssm_rccl_unique_id", C.c_int, [C.c_void_p]),
    ("cssm_rccl_comm_create", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    ("cssm_rccl_comm_destroy", None, [C.c_void_p]),
    ("cssm_pf_shard_series_rccl", C.c_int, [_h, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_size_t, _u8p, C.c_int64,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    ("cssm_pf_shard_spec_segment", C.c_int64, [_h, C.c_int64]),
    ("cssm_pf_shard_unit", C.c_int64, [_h]),
    ("cssm_pf_shard_boundary_pack", C.c_int, [_h, C.c_int, C.c_int, C.c_int64, C.c_void_p]),
    ("cssm_pf_shard_adopt_spec", C.c_int, [_h, C.c_void_p, C.c_int, C.c_int, C.c_int64]),
    ("cssm_pf_shard_resume", C.c_int, [_h, C.POINTER(C.c_uint32)]),
    ("cssm_pf_shard_resume_level", C.c_int, [_h, C.POINTER(C.c_uint32)]),
    ("cssm_pf_shard_peer_setup", C.c_int, [_h, C.c_int, C.c_int, C.c_int64, C.POINTER(PeerHandle)]),
    ("cssm_pf_shard_peer_connect", C.c_int, [_h, C.POINTER(PeerHandle), C.c_int]),
    ("cssm_pf_shard_peer_handshake", C.c_int, [_h, C.c_uint32]),
    ("cssm_pf_shard_peer_probe_stale", C.c_uint32, [_h]),
    ("cssm_pf_shard_peer_close", None, [_h]),
    ("cssm_pf_shard_pack_peer", C.c_int, [_h, C.c_int, C.c_int, C.c_int64]),
    ("cssm_pf_shard_pack_rows_peer", C.c_int, [_h, C.c_int, C.c_int, C.c_int64]),
    ("cssm_pf_shard_peer_rows", C.c_int, [_h, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("cssm_pf_shard_peer_debug", C.c_int64, [_h, C.POINTER(C.c_uint32), C.c_size_t]),
    ("cssm_pf_shard_adopt_peer", C.c_int, [_h, C.c_int, C.c_int, C.c_int64]),
    ("cssm_pf_shard_exchange_peer", C.c_int, [_h, C.c_int, C.c_int, C.c_int64]),
    ("cssm_pf_shard_series_peer", C.c_int, [_h, C.c_int, C.c_int, C.c_size_t, C.c_size_t, _u8p, C.c_int64]),
    ("cssm_pmmh_run", C.c_int, [_h, _descp, _dp, C.c_size_t, C.c_double, _dp, _dp, _u8p, C.c_size_t,
                                C.c_uint64, C.c_size_t, _dp, _dp, _i32p, _dp]),
    ("cssm_pfb_create", C.c_int, [_descp, C.c_uint64, C.c_int, C.c_int, C.POINTER(_h)]),
    ("cssm_pfb_destroy", None, [_h]),
    ("cssm_pfb_num_chains", C.c_int, [_h]),
    ("cssm_pfb_chain", _h, [_h, C.c_int]),
    ("cssm_pfb_filter", C.c_int, [_h, C.POINTER(_descp), _u64p, _dp, _dp, _u8p, C.c_size_t, _dp, _dp, C.POINTER(C.c_int)]),
    ("cssm_pmmh_run_batched", C.c_int, [_h, _descp, _dp, C.c_size_t, C.c_double, _dp, _dp, _u8p, C.c_size_t, _u64p, C.c_size_t, _dp, _dp, _i32p, _dp]),
    ("cssm_pmmh_run_speculative", C.c_int, [_h, _descp, _dp, C.c_size_t, C.c_double, _dp, _dp, _u8p, C.c_size_t, C.c_uint64, C.c_size_t, _dp, _dp, _i32p, _dp]),
    ("cssm_fleet_create", C.c_int, [_descp, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(_h)]),
    ("cssm_fleet_destroy", None, [_h]),
    ("cssm_fleet_num_series", C.c_uint32, [_h]),
    ("cssm_fleet_num_particles", C.c_uint64, [_h]),
    ("cssm_fleet_set_params", C.c_int, [_h, C.POINTER(_descp)]),
    ("cssm_fleet_reseed", C.c_int, [_h, _u64p]),
    ("cssm_fleet_set_option", C.c_int, [_h, C.c_int, C.c_int]),
    ("cssm_fleet_ll_filter", C.c_int, [_h, _u64p, _dp, _dp, _u8p, _dp, _dp, _i32p, C.POINTER(C.c_int)]),
    ("cssm_fleet_filter", C.c_int, [_h, _u64p, _dp, _dp, _u8p, _dp, _dp, _i32p, _dp, _dp, C.POINTER(C.c_int)]),
    ("cssm_fleet_filter_intervals", C.c_int, [_h, _u64p, _dp, _dp, _u8p, C.c_double, _dp, _dp, _i32p, _dp, _dp, _dp, _dp, _dp, _dp, C.POINTER(C.c_int)]),
    ("cssm_fleet_step_intervals", C.c_int, [_h, _u8p, _dp, _dp, _u8p, C.c_double, _dp, _i32p, _dp, _dp, _dp, _dp, _dp, _dp, C.POINTER(C.c_int)]),
    ("cssm_fleet_filter_forecasts", C.c_int, [_h, _u64p, _dp, _dp, _u8p, _u64p, C.c_double, _dp, _dp, _i32p, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp,
                                              _i32p, _i32p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("cssm_fleet_step_forecast", C.c_int, [_h, _u8p, _dp, _dp, _u8p, _u64p, C.c_double, _dp, _i32p, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp,
                                           _i32p, _i32p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("cssm_fleet_pmmh_run", C.c_int, [_h, _descp, _dp, C.c_size_t, C.c_double, _u64p, _dp, _dp, _u8p, _u64p, C.c_size_t, _dp, _dp, _i32p, _dp]),
    ("cssm_fleet_pmmh_last_split", C.c_int, [_h, _dp]),
    ("cssm_fleet_init", C.c_int, [_h, _dp]),
    ("cssm_fleet_step", C.c_int, [_h, _u8p, _dp, _dp, _u8p, _dp, _i32p, C.POINTER(C.c_int)]),
    ("cssm_fleet_summary", C.c_int, [_h, C.c_double, _dp, _dp, _dp, _dp, _dp, _dp]),
    ("cssm_fleet_get_particles", C.c_int, [_h, C.c_uint32, _dp]),
    ("cssm_fleet_get_ancestors", C.c_int, [_h, C.c_uint32, _u32p]),
    ("cssm_fleet_last_ms", C.c_int, [_h, _dp]),
    ("cssm_fleet_forecast", C.c_int, [_h, _u64p, _dp, _u64p, C.c_double, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, C.POINTER(C.c_int)]),
    ("cssm_fleet_forecast_posterior", C.c_int, [_h, _descp, _u64p, _dp, C.c_size_t, _dp, _dp, _u64p, _dp, _u32p, _u64p, C.c_double,
                                                _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _u32p, C.POINTER(C.c_int)]),
    ("cssm_fleet_simulate", C.c_int, [_h, C.c_uint64, _dp, _u64p, _dp, _u64p, _dp, C.POINTER(C.c_int)]),
    ("cssm_fleet_simulate_last_ms", C.c_int, [_h, _dp]),
    ("cssm_fleet_interpolate", C.c_int, [_h, _u64p, _dp, _dp, _u8p, C.c_double, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp, C.POINTER(C.c_int)]),
    ("cssm_fleet_interpolate_last_ms", C.c_int, [_h, _dp]),
    ("cssm_fleet_smooth", C.c_int, [_h, _u64p, _dp, _dp, _u8p, C.c_uint32, C.c_double, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _u32p,
                                    C.POINTER(C.c_int)]),
    ("cssm_fleet_smooth_last_ms", C.c_int, [_h, _dp]),
    ("cssm_fleet_if2", C.c_int, [_h, _descp, _dp, _dp, C.c_size_t, _dp, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, _u64p, _u64p, _dp, _dp, _u8p,
                                 _dp, _dp, _dp, _dp, _i32p, _dp, _u32p, C.POINTER(C.c_int)]),
    ("cssm_fleet_if2_last_ms", C.c_int, [_h, _dp]),
    ("cssm_fleet_if2_cooling", C.c_int, [C.c_double, C.c_uint32, C.c_uint32, _dp]),
    ("cssm_fleet_if2_layout", C.c_int, [_descp, _i32p, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("cssm_fleet_pmmh_chains", C.c_int, [_h, _descp, _dp, C.c_size_t, _dp, C.c_int, C.c_void_p, _dp, _dp, C.c_uint32, C.c_uint32, C.c_uint32,
                                         _u64p, _u64p, _dp, _dp, _u8p, _dp, _dp, _i32p, _dp, _u32p, C.POINTER(C.c_int)]),
    ("cssm_fleet_pmmh_chains_last_ms", C.c_int, [_h, _dp]),
    ("cssm_fleet_pmmh_chains_lgcp", C.c_int, [_h, _descp, _dp, C.c_size_t, _dp, C.c_int, C.c_void_p, _dp, _dp, C.c_uint32, C.c_uint32, C.c_uint32,
                                              _u64p, _u64p, _dp, _dp, _dp, _i32p, _dp, _u32p, C.POINTER(C.c_int)]),
    ("cssm_fleet_pmmh_chains_lgcp_last_ms", C.c_int, [_h, _dp]),
    ("cssm_fleet_pmmh_lgcp_pack_record", C.c_int, [_descp, C.c_double, C.c_double, C.c_uint32, _u8p, C.c_size_t, C.POINTER(C.c_size_t), _dp,
                                                   C.c_size_t, C.POINTER(C.c_size_t)]),
    ("cssm_fleet_window", C.c_int, [_h, C.c_uint32]),
    ("cssm_fleet_window_depth", C.c_uint32, [_h, C.c_uint32]),
    ("cssm_fleet_step_interpolate", C.c_int, [_h, _u8p, _dp, _dp, _u8p, _u32p, C.c_uint32, C.c_double, _dp, _i32p, _u32p, _dp, _dp, _dp, _dp, _dp, _dp,
                                              C.POINTER(C.c_int)]),
    ("cssm_fleet_step_interpolate_last_ms", C.c_int, [_h, _dp]),
    ("cssm_fleet_observation_index", C.c_uint64, [_h, C.c_uint32]),
    ("cssm_fleet_pack_record", C.c_int, [_descp, C.c_uint64, C.c_uint64, C.c_double, C.c_double, C.c_double, C.c_int, C.c_uint32,
                                         _u8p, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("cssm_fleet_create_lgcp", C.c_int, [_descp, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(_h)]),
    ("cssm_fleet_pack_record_lgcp", C.c_int, [_descp, C.c_uint64, C.c_uint64, C.c_double, C.c_double, C.c_uint32, _u8p, C.c_size_t,
                                              C.POINTER(C.c_size_t), _dp, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("cssm_fleet_init_from", C.c_int, [_h, _u8p, _dp, _u64p, _dp, _u32p, _u64p, _u32p, C.POINTER(C.c_int)]),
    ("cssm_fleet_copy_series", C.c_int, [_h, _h, _u64p, C.c_int, C.POINTER(C.c_int)]),   # (map: int64 entries, -1 = keep, in the header's uint64_t)
    ("cssm_fleet_ll_filter_more", C.c_int, [_h, _u64p, _dp, _dp, _u8p, _dp, _dp, _i32p, C.POINTER(C.c_int)]),
    ("cssm_fleet_filter_intervals_more", C.c_int, [_h, _u64p, _dp, _dp, _u8p, C.c_double, _dp, _dp, _i32p, _dp, _dp, _dp, _dp, _dp, _dp,
                                                   C.POINTER(C.c_int)]),
    ("cssm_diag_copy_ceiling", C.c_int,[C.c_int, C.c_size_t, C.c_int, _dp]),
    ("cssm_contract_eval", C.c_int, [C.c_int, C.c_int, _dp, C.c_size_t, _dp, C.c_size_t]),
    ("cssm_desc_flatten", C.c_int, [_descp, _dp, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("cssm_last_error", C.c_char_p, []),
    ("cssm_version", C.c_char_p, []),
]

_lib = None


def load_library(path: str | None = None) -> C.CDLL:
    """dlopen libcssm_pf.so and bind every declared symbol.  Fails loudly if it is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise ImportError(
            f"{p} not found: the HIP extension is not built. Run `python -c \"import __graft_entry__ "
            "as g; g.build()\"` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = C.CDLL(p, mode=C.RTLD_GLOBAL)
    for name, res, args in SYMBOLS:
        fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def last_error() -> str:
    msg = load_library().cssm_last_error()
    return msg.decode() if msg else ""


def check(rc: int) -> None:
    if rc != 0:
        msg = load_library().cssm_last_error()
        raise CssmError(rc, msg.decode() if msg else "")
