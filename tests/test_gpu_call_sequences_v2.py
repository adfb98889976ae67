"""-m gpu: the second vocabulary of the call-sequence tests (tests/call_sequences.py, "V2") on REUSED handles: the calls that form rows
inside the filtering call (cssm_pf_filter_intervals / _more / cssm_pf_step_intervals, cssm_pf_filter_forecasts / _more /
cssm_pf_step_forecast), cssm_pf_smooth, and cssm_pmmh_run on a handle that lives on -- behind propagate / adopt, init_from, set_params,
reseed, a failed step, a run of more than 1024 records, option switches and each other.  Their own files compare them with the route
they replaced on fresh handles; here every expectation comes from the fresh-replay oracle, as in tests/test_gpu_call_sequences.py:

  intervals   the oracle's init; summary; (step; summary)*
  forecasts   row s against test_gpu_forecast.expected from the oracle's cloud BEFORE record s under the key the reference derives
              (cssm_pf_run_key(seed, 2^63 | observation index), so a reseed or a restart in between shows), the PIT counts against numpy
  smooth      ll of the oracle's interpolate, the sequential twin's trajectories on the oracle's history, the oracle's summaries of them
  pmmh        OraclePf.pmmh

tests/test_call_sequences_host.py computes the coverage of the committed list; the hand-written sequences below aim at one carried
field each.  The mutations tried against these sequences are listed in DESIGN.md section 7."""
from __future__ import annotations

import pytest

import call_sequences as cs
from call_sequences import op
from test_gpu_call_sequences import BIG, drive, twin      # noqa: F401  (twin: the module-scoped fixture of the first half)

pytestmark = pytest.mark.gpu

FAST = [s for s in cs.committed_sequences_v2() if not s[4]]
SLOW = [s for s in cs.committed_sequences_v2() if s[4]]


@pytest.mark.parametrize("case", FAST, ids=[s[0] for s in FAST])
def test_seeded_v2_sequence_matches_the_fresh_oracle(case, twin, monkeypatch):
    """Group sums from two units on (CSSM_GRP_MIN_UNITS, read once when the handle is created)."""
    monkeypatch.setenv("CSSM_GRP_MIN_UNITS", "2")
    _, name, n, ops, _ = case
    drive(name, n, ops, twin)


@pytest.mark.slow
@pytest.mark.parametrize("case", SLOW, ids=[s[0] for s in SLOW])
def test_seeded_v2_sequence_through_the_grid_stride_loops(case, twin):
    """300001 particles: the grid-stride loops of the summary take more than one turn."""
    _, name, n, ops, _ = case
    drive(name, n, ops, twin)


# ----------------------------------------------------------------------------- hand-written: one carried field each
HAND_V2 = {
    # anc_valid is false behind cssm_pf_adopt: the row's source is the cloud itself, not the cloud through the last native ancestors
    "forecast_row_through_identity_ancestors_behind_adopt": ("c2", 5000, [
        op("init", 0.0), op("step", 1.0, 2.0, 1), op("step", 2.0, 1.0, 1), op("propagate", 3.0, 2.0, 1), op("adopt", 0.3125),
        op("step_forecast", 4.0, 3.0, 1, None, 0.975), op("particles"), op("propagate", 5.0, 1.0, 1), op("adopt", 0.0),
        op("step_forecast", 5.0, 2.0, 1, 0xABCDEF, 0.9), op("ancestors"), op("particles")]),
    "interval_rows_through_identity_ancestors_behind_adopt": ("c3", 4097, [
        op("init", 0.0), op("step", 1.0, 2.0, 1), op("propagate", 2.0, 1.0, 1), op("adopt", 0.9990234375),
        op("run_intervals_more", 4, 3, 0.975, None), op("particles"), op("propagate", 9.0, 1.0, 1), op("adopt", 0.3125),
        op("run_forecasts_more", 3, 5, 0, 1.0, None), op("particles")]),
    # a weighted propagate that is never adopted: the proposed cloud is the current one, the log-weights stand in `logw`
    "step_intervals_behind_a_weighted_propagate_without_adopt": ("c2", 5000, [
        op("init", 0.0), op("step", 1.0, 2.0, 1), op("propagate", 2.0, 3.0, 1), op("step_intervals", 3.0, 1.0, 1, 0.9), op("weights"),
        op("propagate", 4.0, 1.0, 1), op("step_forecast", 4.5, 2.0, 1, None, 0.975), op("particles")]),
    # recs_cap and the rows' scratch: buffers regrown by a long plain series, then a short rows call
    "forecasts_more_of_3_behind_a_run_of_1035": ("c2", 513, [
        op("run", 1035, 4, 0), op("run_forecasts_more", 3, 7, 0, 0.975, None), op("forecast_key"),
        op("step_forecast", 4000.0, 1.0, 1, None, 0.975), op("particles")]),
    # the smoother borrows the handle's buffers and keeps the history of T + 1 clouds: nothing of it may show in the next series
    "interval_rows_behind_a_smooth_of_12": ("c2", 1000, [
        op("smooth", 12, 4, 64, 0.975), op("refused", "ESTATE", op("run_intervals_more", 2, 5, 0.975, None)), op("init", 0.0),
        op("run_intervals_more", 5, 6, 0.9, 2), op("particles")]),
    "smooth_of_3_behind_a_smooth_of_12": ("c2", 5000, [
        op("smooth", 12, 4, 64, 0.975), op("smooth", 3, 5, 64, 0.9), op("smooth", 12, 6, 7, 1.0), op("init", 0.0),
        op("step_intervals", 1.0, 2.0, 1, 0.975), op("particles")]),
    # cssm_pmmh_run leaves its last proposal's parameters and key: set_params and reseed must both reach the next cloud and its default keys
    "default_keys_behind_pmmh_set_params_reseed": ("c2", 1000, [
        op("init", 0.0), op("step", 1.0, 2.0, 1), op("pmmh", 5, 3, 3, 0.01, 77), op("set_params", 1), op("reseed", 555),
        op("run_forecasts", 4, 8, 0, 0.975, None), op("forecast_key"), op("pmmh", 3, 4, 2, 0.0025, 78), op("reseed", 556), op("set_params", 0),
        op("run_intervals", 3, 9, 0.9, None), op("particles")]),
    # the held record's row is formed behind its redo, whichever kernels the options select (wmode follows the redone record)
    "held_record_in_forecasts_more_behind_fused_sums_off": ("c2", 5000, [
        op("init", 0.0), op("step", 1.0, 2.0, 1), op("set_option", 3, 0), op("run_forecasts_more", 5, 3, 0, 0.975, 2), op("logw"),
        op("set_option", 3, 1), op("run_forecasts_more", 4, 4, 1, 0.9, 3), op("particles")]),
    "held_record_in_forecasts_more_behind_whole_tiles": ("c2", BIG, [
        op("init", 0.0), op("set_option", 6, 2), op("run_forecasts_more", 3, 3, 0, 0.975, 1), op("particles")]),
    "held_record_in_forecasts_more_behind_wave_sums": ("c1", BIG, [
        op("set_option", 6, 1), op("set_option", 10, 2), op("init", 0.0), op("run_forecasts_more", 3, 3, 0, 0.975, 2), op("particles")]),
    # the level predicted from the last max of one series must not reach the first row behind a NEW cloud (Scalars::next_ref)
    "lgcp_level_does_not_survive_a_new_cloud_in_interval_rows": ("c4p1", 5000, [
        op("run_intervals", 6, 1, 0.975, None), op("init", 0.0), op("run_intervals_more", 4, 2, 0.9, None), op("particles"),
        op("run_intervals", 3, 3, 1.0, None), op("step_intervals", 1.0, 1.0, 1, 0.975), op("particles")]),
    # a step that failed half-way, then the handle as new: the rows call behind it starts from the new cloud at its own clock
    "forecasts_more_behind_a_failed_step_forecast": ("c1", 513, [
        op("init", 1.0), op("step", 2.0, 2.0, 1), op("fails", "ENONFINITE", op("step_forecast", 0.0, 2.0, 1, None, 0.975)), op("init", 0.0),
        op("run_forecasts_more", 3, 5, 0, 0.975, None), op("fails", "ENONFINITE", op("step_intervals", -1.0, 1.0, 1, 0.9)),
        op("run_intervals", 3, 6, 0.975, None), op("particles")]),
}


@pytest.mark.parametrize("name", sorted(HAND_V2))
def test_hand_written_v2_sequence(name, twin, monkeypatch):
    monkeypatch.setenv("CSSM_GRP_MIN_UNITS", "2")
    spec_name, n, ops = HAND_V2[name]
    drive(spec_name, n, ops, twin)
