"""-m gpu: REUSED handles driven through sequences of public calls (tests/call_sequences.py), the expected result of every call
computed from a FRESH oracle that replays the live prefix, bit for bit.

Every other parity test creates a handle, runs one scenario and closes it.  The product is used the other way round: PMMH
re-parameterises and re-runs one handle thousands of times, the streaming Filter steps one handle for ever and asks for summaries
and forecasts in between, the batch handle is re-filled per iteration -- and cssm_pf_set_option switches the launch geometry with
no look at what the running filter left behind, under the header's promise that results are bit-identical in every setting.
The seeded sequences cover the vocabulary (tests/test_call_sequences_host.py computes the coverage and checks the expectation
itself without a GPU); the hand-written ones below aim at the carried fields of csrc/cssm_internal.h one by one.

Mutations tried against these sequences (one carried field broken per scratch build, values only, never an extent or a launch
geometry) and what caught each are listed in DESIGN.md section 7."""
from __future__ import annotations

import os
import subprocess
import sys
import time

import numpy as np
import pytest

import call_sequences as cs
import cases
from call_sequences import op
from composablestatespacemodels_amd.filter import NativePf, NativePfBatch
from oracle import oracle

pytestmark = pytest.mark.gpu

SEED = cases.SEED
BIG = 70 * 1024 + 3


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    from test_forecast_draws import build_twin      # (the host twin of include/cssm_obs_draws.h, as tests/test_gpu_forecast.py uses it)
    return build_twin(tmp_path_factory.mktemp("twin"))


def drive(spec_name, n, ops, twin, seed=SEED):
    spec = cs.SPECS[spec_name]
    make = lambda model, s: NativePf(model, n, s, lgcp_precision=spec.precision)
    g = make(spec.model(0), seed)
    try:
        return cs.run_sequence(g, spec_name, n, seed, ops, twin=twin, make_subject=make)
    finally:
        g.close()


FAST = [s for s in cs.committed_sequences() if not s[4]]
SLOW = [s for s in cs.committed_sequences() if s[4]]


@pytest.mark.parametrize("case", FAST, ids=[s[0] for s in FAST])
def test_seeded_sequence_matches_the_fresh_oracle(case, twin, monkeypatch):
    """Group sums from one unit on (CSSM_GRP_MIN_UNITS, read once when the handle is created): with options 6 = 1, 2, 3 in the
    vocabulary these sizes reach the kernels of the large clouds."""
    monkeypatch.setenv("CSSM_GRP_MIN_UNITS", "1")
    _, name, n, ops, _ = case
    drive(name, n, ops, twin)


@pytest.mark.slow
@pytest.mark.parametrize("case", SLOW, ids=[s[0] for s in SLOW])
def test_seeded_sequence_at_the_native_thresholds(case, twin):
    """2^20 particles and just beyond, no override: the geometry, the group sums and the wave sums switch where the library says."""
    _, name, n, ops, _ = case
    drive(name, n, ops, twin)


# ----------------------------------------------------------------------------- hand-written: one carried field each
HAND = {
    # opt_whole / split switched between the steps of one series: the cloud's layout (src / src2 / n_split), the sums the last
    # propagate left (last_grp, grp_layout) and the max-slot rotation must survive the change of geometry
    "whole_tiles_0_2_0_within_a_series": ("c2", BIG, [
        op("init", 0.0), op("step", 1.0, 2.0, 1), op("step", 2.0, 1.0, 1),
        op("set_option", 6, 2), op("step", 3.0, 3.0, 1), op("particles"), op("step", 3.5, 0.0, 0), op("step", 4.0, 2.0, 1),
        op("set_option", 6, 0), op("step", 5.0, 1.0, 1), op("ancestors"), op("step", 6.0, 2.0, 1), op("summary", 0.9), op("particles")]),
    "whole_tiles_1_3_within_a_batch_series": ("c1", BIG, [
        op("set_option", 6, 1), op("run", 5, 3, 0), op("set_option", 6, 3), op("run_more", 4, 8), op("last_device_us"),
        op("set_option", 6, 1), op("step", 20.0, 2.0, 1), op("set_option", 7, 0), op("step", 21.0, 1.0, 1), op("particles")]),
    # wmode: which of weights / log-weights `logw` holds follows the LAST weighted step, whatever the option says now
    "fused_sums_switched_between_two_steps": ("c2", 5000, [
        op("init", 0.0), op("step", 1.0, 2.0, 1), op("weights"), op("logw"),
        op("set_option", 3, 0), op("weights"), op("step", 2.0, 1.0, 1), op("logw"), op("weights"),
        op("set_option", 3, 1), op("logw"), op("step", 3.0, 3.0, 1), op("weights"), op("logw"), op("particles")]),
    # (found by these tests) an observation WITHOUT a datum through cssm_pf_propagate stores no log-weights, but flagged the buffer
    # as holding them: cssm_pf_get_logw then handed out the fused step's weights as log-weights
    "unweighted_propagate_keeps_the_weight_mode": ("c2", 5000, [
        op("init", 0.0), op("step", 1.0, 2.0, 1), op("weights"), op("propagate", 2.0, 0.0, 0), op("weights"), op("logw"),
        op("particles"), op("step", 3.0, 1.0, 1), op("weights"), op("particles")]),
    # last_ws / last_grp: the wave sums and group sums of the native step before a cloud the HOST replaced
    "wave_sums_then_a_host_resampled_step": ("c1", BIG, [
        op("set_option", 6, 1), op("set_option", 10, 2), op("init", 0.0), op("step", 1.0, 2.0, 1), op("step", 2.0, 1.0, 1),
        op("propagate", 3.0, 2.0, 1), op("adopt", 0.3125), op("step", 4.0, 3.0, 1), op("ancestors"), op("step", 5.0, 1.0, 1),
        op("propagate", 6.0, 1.0, 1), op("adopt", 0.0), op("run_more", 4, 5), op("particles")]),
    # recs_cap / path_cap / done_seq: series lengths that grow, shrink, and continue beyond every earlier one
    "series_40_then_3_then_60_more": ("c2", 1000, [
        op("run", 40, 1, 1), op("run", 3, 2, 1), op("run_more", 60, 3), op("last_device_us"), op("summary", 0.5),
        op("run", 1100, 4, 1), op("run", 1, 5, 1), op("run_more", 1, 6), op("last_device_us"), op("particles")]),
    # the model of the first step is the one set AFTER the cloud was drawn (the cloud itself keeps the old m0 / c0)
    "set_params_between_init_and_the_first_step": ("c2", 5000, [
        op("init", 0.0), op("set_params", 2), op("step", 1.0, 2.0, 1), op("particles"), op("set_params", 0), op("step", 2.0, 2.0, 1),
        op("refused", "EINVAL_DESC", op("set_params_other")), op("step", 3.0, 1.0, 1), op("particles")]),
    # the key of the NEXT transition changes between the two halves of a split step; the adopted cloud does not depend on it
    "reseed_between_propagate_and_adopt": ("c3", 1025, [
        op("init", 0.0), op("step", 1.0, 2.0, 1), op("propagate", 2.0, 1.0, 1), op("reseed", 424242), op("forecast", 2, None, 0.9, 0),
        op("adopt", 0.9990234375), op("step", 3.0, 2.0, 1), op("forecast_key"), op("particles")]),
    # have_level / the predicted level behind a batch call, then an observation whose level the max rules out (redone in the call)
    "outlier_directly_after_run_more": ("negbin", 5000, [
        op("run", 6, 1, 0), op("run_more", 5, 2), op("step", 30.0, 400.0, 1), op("logw"), op("weights"), op("step", 31.0, 2.0, 1),
        op("weights"), op("run_more", 3, 9), op("particles")]),
    "lgcp_long_gap_directly_after_run_more": ("c4p1", 5000, [
        op("run", 5, 1, 0), op("run_more", 4, 2), op("step", 6.0, 1.0, 1), op("weights"), op("step", 6.125, 1.0, 1), op("logw"),
        op("propagate", 6.25, 1.0, 1), op("adopt", 0.3125), op("step", 6.5, 1.0, 1), op("particles")]),
    # the level predicted from the last max of one series must not reach the first observation behind a NEW cloud (Scalars::next_ref)
    "lgcp_level_does_not_survive_a_new_cloud": ("c4p1", 5000, [
        op("run", 6, 1, 0), op("init", 0.0), op("run_more", 4, 2), op("particles"), op("run", 5, 3, 1), op("init_from", 0.0, 0.25),
        op("run_more", 3, 4), op("weights"), op("step", 1.5, 1.0, 1), op("particles")]),
    # a continued call that STARTS on a missing observation reports the ESS the handle had: N behind a new cloud, the host's
    # behind an adopted one (ess_host), never the one of the series before (data seeds 3 and 5: has[0] = 0)
    "unweighted_first_observation_of_a_continued_call": ("c2", 5000, [
        op("run", 8, 1, 0), op("init", 0.0), op("run_more", 3, 3), op("particles"), op("step", 9.0, 2.0, 1), op("init_from", 1.0, 0.5),
        op("run_more", 4, 5), op("propagate", 12.0, 3.0, 1), op("adopt", 0.3125), op("run_more", 3, 3), op("particles")]),
    # N equal values: every rank of the radix selection lands in one bucket
    "summary_directly_after_init_from": ("c3", 5000, [
        op("init_from", 1.0, 0.25), op("summary", 0.975), op("summary", 1.0), op("summary", 0.25 / 5000), op("step", 1.0, 2.0, 1),
        op("summary", 0.5), op("particles")]),
    # a series that failed half-way, then the handle as new; refusals leave it as it was
    "a_failed_series_then_a_fresh_start": ("c1", 1025, [
        op("refused", "ESTATE", op("step", 1.0, 1.0, 1)), op("refused", "ESTATE", op("summary", 0.975)), op("refused", "ESTATE", op("run_more", 2, 5)),
        op("init", 1.0), op("step", 2.0, 2.0, 1), op("refused", "EINVAL_ARG", op("run", 0, 0, 0)), op("refused", "EINVAL_ARG", op("set_option", 2, 7)),
        op("step", 3.0, 1.0, 1), op("fails", "ENONFINITE", op("step", 1.0, 2.0, 1)), op("run", 7, 3, 1), op("step", 20.0, 1.0, 1),
        op("fails", "ENONFINITE", op("step", 2.0, 2.0, 1)), op("init", 0.0), op("step", 1.0, 2.0, 1), op("weights"), op("particles")]),
    # an interpolation borrows the handle's buffers: afterwards nothing runs until a new cloud is drawn, then everything does
    "interpolate_then_a_new_cloud": ("c2", 1025, [
        op("init", 0.0), op("step", 1.0, 2.0, 1), op("interpolate", 9, 4, 0.9), op("refused", "ESTATE", op("step", 30.0, 1.0, 1)),
        op("refused", "ESTATE", op("summary", 0.9)), op("set_option", 6, 1), op("run", 4, 2, 1), op("step", 12.0, 2.0, 1), op("particles")]),
    # the three kernels of option 8 on a structure outside the ahead-of-time table, switched inside one series
    "specialise_1_0_2_within_a_series": ("rtc", 5000, [
        op("init", 0.0), op("step", 1.0, 2.0, 1), op("set_option", 8, 0), op("step", 2.0, 1.0, 1), op("set_option", 8, 2),
        op("step", 3.0, 3.0, 1), op("set_option", 8, 1), op("run_more", 5, 3), op("particles")]),
    # a new resampler draws a new cloud; stratified and multinomial series on a handle that ran systematic ones
    "resamplers_in_turn": ("c2", 5000, [
        op("run", 5, 1, 0), op("set_option", 2, 2), op("run", 5, 1, 1), op("logw"), op("step", 9.0, 2.0, 1), op("set_option", 2, 1),
        op("init", 0.0), op("step", 1.0, 2.0, 1), op("weights"), op("set_option", 2, 0), op("run", 4, 7, 1), op("particles")]),
}


def test_the_hand_written_data_are_what_their_comments_say():
    for T, dseed in ((3, 3), (4, 5)):
        assert cs.series(cs.SPECS["c2"], T, dseed, 0.0, True)[2][0] == 0


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_written_sequence(name, twin, monkeypatch):
    monkeypatch.setenv("CSSM_GRP_MIN_UNITS", "1")
    spec_name, n, ops = HAND[name]
    drive(spec_name, n, ops, twin)


def test_the_runner_names_the_op_on_a_real_handle(twin):
    """The report of a divergence, on the GPU: a subject whose reseed never reaches the library."""
    class Deaf(NativePf):
        def reseed(self, seed):
            self.seed = int(seed)
    spec = cs.SPECS["c2"]
    g = Deaf(spec.model(0), 2000, SEED)
    seq = [op("init", 0.0), op("step", 1.0, 2.0, 1), op("reseed", 99), op("step", 2.0, 1.0, 1), op("particles")]
    with pytest.raises(cs.Divergence) as e:
        cs.run_sequence(g, "c2", 2000, SEED, seq, twin=twin, make_subject=lambda m, s: NativePf(m, 2000, s))
    msg = str(e.value)
    assert "op 3 op('step', 2.0, 1.0, 1)" in msg and "a FRESH handle replaying the live prefix" in msg and "matches the oracle" in msg
    g.close()


# ----------------------------------------------------------------------------- the device time of a continued call
_CHILD = r"""
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import call_sequences as cs
from call_sequences import op
from composablestatespacemodels_amd.filter import NativePf
seq = [op("run", 6, 1, 0), op("run_more", 5, 2), op("last_device_us"), op("step", 30.0, 2.0, 1), op("run_more", 1, 3), op("last_device_us"),
       op("init", 0.0), op("run_more", 20, 4), op("last_device_us"), op("run_more", 3, 5), op("last_device_us"), op("particles")]
g = NativePf(cs.SPECS["c2"].model(0), 5000, 20260101)
cs.run_sequence(g, "c2", 5000, 20260101, seq)
g.close()
print("child ok")
"""


def test_last_device_us_never_spans_more_than_its_call_on_the_copy_path():
    """CSSM_UPLOAD_MEMCPY=1 (read once per PROCESS, at the first record upload): the records travel by hipMemcpyAsync and no kernel
    stamps the call's first instruction.  cssm_pf_last_device_us must then say CSSM_ESTATE, or an interval within the call's wall
    time -- never one that starts at an earlier call's stamp.  A fresh child process, so that the switch is read with the variable set."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, CSSM_UPLOAD_MEMCPY="1")
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=os.path.dirname(here), tests=here)], env=env, timeout=300,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-4000:]


def test_last_device_us_of_every_continued_call(twin):
    """... and on the default path every continued call reports 0 < device time <= its own wall time, whatever ran before it."""
    seq = [op("run", 6, 1, 0), op("run_more", 5, 2), op("last_device_us"), op("step", 30.0, 2.0, 1), op("summary", 0.9), op("run_more", 1, 3),
           op("last_device_us"), op("init", 0.0), op("run_more", 20, 4), op("last_device_us"), op("propagate", 40.0, 1.0, 1), op("adopt", 0.0),
           op("run_more", 3, 5), op("last_device_us"), op("particles")]
    r = drive("c2", 5000, seq, twin)
    g = NativePf(cs.SPECS["c2"].model(0), 5000, SEED)
    t, y, has = cs.series(cs.SPECS["c2"], 4, 1, 0.0, False)
    g.run(t, y, has)
    t2, y2, has2 = cs.series(cs.SPECS["c2"], 3, 2, float(t[-1]), True)
    t0 = time.perf_counter(); g.run_more(t2, y2, has2); wall = (time.perf_counter() - t0) * 1e6
    assert 0.0 < g.last_device_us() <= wall
    g.close()
    assert r.wall_us is not None


# ----------------------------------------------------------------------------- the batch handle, re-filled
def test_a_batch_handle_refilled_three_times_equals_fresh_single_handles(twin):
    """NativePfBatch.filter three times on ONE batch handle with other models, keys and series lengths each time (longer, shorter,
    longer than every earlier one): each chain equal to a fresh single handle and to a fresh oracle; then the views."""
    spec = cs.SPECS["c2"]
    n, B = 5000, 3
    b = NativePfBatch(spec.model(0), n, B)
    fills = [((0, 1, 2), (SEED, SEED + 1, 7), 9, 11), ((3, 0, 1), (5, SEED, SEED + 9), 2, 12), ((2, 2, 0), (SEED + 3, 8, 1), 14, 13)]
    for ks, seeds, T, dseed in fills:
        models = [spec.model(k) for k in ks]
        t, y, has = cs.series(spec, T, dseed, 0.0, False)
        ll, path, rc = b.filter(models, seeds, t, y, has)
        assert not rc.any()
        for k in range(B):
            o = oracle.OraclePf(models[k].descriptor(), n, seeds[k])
            ol, _, _, opath = o.filter(t, y, has, want_path=True)
            with NativePf(models[k], n, seeds[k]) as g:
                gl, _, _, gpath = g.run(t, y, has, want_path=True)
                assert ll[k] == ol == gl, (T, k, ll[k], ol, gl)
                np.testing.assert_array_equal(path[k], opath); np.testing.assert_array_equal(gpath, opath)
            v = b.chain(k)
            np.testing.assert_array_equal(v.particles(), o.particles(), err_msg=f"T = {T}, chain {k}")
            np.testing.assert_array_equal(v.ancestors(), o.ancestors(), err_msg=f"T = {T}, chain {k}")
    # the views after the last fill: summaries and forecasts of every chain's cloud
    from test_gpu_forecast import check_forecast, expected
    for k in range(B):
        v = b.chain(k)
        o = oracle.OraclePf(models[k].descriptor(), n, seeds[k]); o.filter(t, y, has)
        gs, os_ = v.summary(0.9), o.summary(0.9)
        for i in (1, 2, 4, 5):
            np.testing.assert_array_equal(gs[i], os_[i])
        np.testing.assert_allclose(gs[0], os_[0], rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(gs[3], os_[3], rtol=1e-12, atol=1e-13)
        times = cs.horizon_times(float(t[-1]), 3)
        r = v.forecast(times, 0xBA7C4 + k, 0.9, want_samples=True)
        check_forecast(r, *expected(models[k], o.particles(), float(t[-1]), times, 0xBA7C4 + k, twin), interval=0.9)
        np.testing.assert_array_equal(v.particles(), o.particles())      # ... which left the chain as it was
    b.close()
