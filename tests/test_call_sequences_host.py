"""The CPU half of the call-sequence tests (tests/call_sequences.py; the GPU half is tests/test_gpu_call_sequences.py).

Nothing here needs a GPU: the generator is deterministic and emits only sequences the documented state machine allows; the
committed seed list covers the vocabulary (a condition the test computes, not a hope); the reference side is sound -- ONE oracle
object carried through a whole sequence equals the fresh replay of its live prefix after every op, bit for bit, so the expectation
the GPU half compares with has no stale state of its own; and the oracle time of the non-slow GPU sequences stays within a budget
that is counted from the sequences themselves."""
from __future__ import annotations

import numpy as np
import pytest

import call_sequences as cs
from call_sequences import op

ALL = cs.committed_sequences()
FAST = [s for s in ALL if not s[4]]


def test_generator_is_deterministic_and_every_sequence_is_legal():
    for seed, name, n, length in cs.SEQUENCES + cs.SLOW_SEQUENCES:
        a, b = cs.sequence(seed, name, n, length), cs.sequence(seed, name, n, length)
        assert a == b and repr(a) == repr(b)
        assert len(a) >= length
        assert eval(cs.pasteable(a), {"op": op}) == a, "a printed sequence pastes back into the same ops"
    assert cs.sequence(1, "c2", 1000, 30) != cs.sequence(2, "c2", 1000, 30)
    for id_, name, n, ops, _ in ALL:
        cs.check_legal(cs.SPECS[name], ops)


def test_the_state_machine_refuses_what_the_header_refuses():
    spec = cs.SPECS["c2"]
    for bad in ([op("step", 1.0, 1.0, 1)],                                            # step before init
                [op("init", 0.0), op("adopt", 0.3)],                                  # adopt without a weighted propagate
                [op("init", 2.0), op("step", 1.0, 1.0, 1)],                           # time before the clock
                [op("init", 0.0), op("logw")],                                        # no weighted step yet
                [op("run", 0, 1, 0)],                                                 # empty data
                [op("interpolate", 3, 1, 0.9), op("step", 9.0, 1.0, 1)],              # the handle must be re-initialised
                [op("init", 0.0), op("set_option", 2, 1), op("step", 1.0, 1.0, 1)],   # a new resampler needs a new cloud
                [op("init", 0.0), op("fails", "ENONFINITE", op("step", -1.0, 1.0, 1)), op("step", 1.0, 1.0, 1)],
                [op("init", 0.0), op("refused", "ESTATE", op("step", 1.0, 1.0, 1))],  # ... it would be accepted
                [op("init", 0.0), op("step", 1.0, 1.0, 1), op("last_device_us")],
                [op("set_option", 6, 4)]):
        with pytest.raises(cs.IllegalSequence):
            cs.check_legal(spec, bad)
    with pytest.raises(cs.IllegalSequence):
        cs.check_legal(cs.SPECS["c4p1"], [op("init", 0.0), op("fails", "ENONFINITE", op("step", -1.0, 1.0, 1))])


def _kinds_of(spec, n, st, o):
    """The kinds an op counts as in the coverage table (before it is applied to `st`)."""
    k = o.kind
    if k == "set_option":
        return [f"opt{o[1]}"]
    if k == "refused":
        return [f"refused:{o[1]}:{o[2].kind}"]
    if k == "fails":
        return ["fails:ENONFINITE"]
    out = [k]
    if k == "step" and not spec.lgcp:
        if not o[3]:
            out.append("step_missing")
        if o[1] == st.t:
            out.append("step_dt0")
        if o[3] and o[2] == spec.outlier:
            out.append("step_outlier")
    if k == "summary":
        out.append("summary_beyond_0.975" if o[1] != 0.975 else "summary_0.975")
        if int(np.floor(o[1] * n)) == 0:
            out.append("summary_rank_clamps")
    if k == "forecast" and o[4]:
        out.append("forecast_chunked")
    if k == "run":
        out.append("run_with_path" if o[3] else "run_ll_only")
        if o[1] == 1:
            out.append("run_T1")
        if o[1] > 1024:
            out.append("run_beyond_1024_records")
    return out


REQUIRED_KINDS = (cs.STATE_KINDS + cs.READ_KINDS + cs.STEP_VARIANTS +
                  ("summary_beyond_0.975", "summary_rank_clamps", "forecast_chunked", "run_with_path", "run_ll_only", "run_T1",
                   "run_beyond_1024_records", "fails:ENONFINITE", "refused:ESTATE:step", "refused:ESTATE:run_more",
                   "refused:ESTATE:summary", "refused:EINVAL_ARG:set_option", "refused:EINVAL_ARG:run", "refused:EINVAL_ARG:run_more",
                   "refused:EINVAL_DESC:set_params_other"))


def test_coverage_of_the_committed_sequences():
    """Every op kind at least 5 times; every ordered pair of state-changing kinds the header allows back to back at least once
    (set_option per option); every documented option value followed by a weighted step before that option changes again; run
    lengths that grow and shrink, with one longer than every earlier one of its sequence."""
    counts = {}
    option_seen = set()
    grows = shrinks = longest_last = 0
    for id_, name, n, ops, _ in ALL:
        spec = cs.SPECS[name]
        st = cs.HostState(spec)
        waiting = {}                     # option -> value that has not seen a weighted step yet
        lengths = []
        for o in ops:
            for k in _kinds_of(spec, n, st, o):
                counts[k] = counts.get(k, 0) + 1
            if o.kind == "set_option" and o[1] in cs.OPTION_VALUES:
                waiting[o[1]] = o[2]
            elif cs.is_weighted_op(spec, st, o):
                option_seen.update(waiting.items())
                waiting.clear()
            if o.kind in ("run", "run_more"):
                lengths.append(o[1])
            st.apply(o)
        grows += sum(b > a for a, b in zip(lengths, lengths[1:]))
        shrinks += sum(b < a for a, b in zip(lengths, lengths[1:]))
        longest_last += any(i >= 2 and L > max(lengths[:i]) and min(lengths[:i]) < max(lengths[:i]) for i, L in enumerate(lengths))
    few = {k: counts.get(k, 0) for k in REQUIRED_KINDS if counts.get(k, 0) < 5}
    assert not few, f"op kinds that occur fewer than 5 times: {few}"
    tab = cs.pair_table([s[3] for s in ALL])
    spec = cs.SPECS[cs.COMPLETION[0]]
    missing = [(a, b) for a in cs.STATE_KINDS for b in cs.STATE_KINDS if cs.pair_allowed(spec, a, b) and (a, b) not in tab]
    assert not missing, f"ordered pairs of state-changing kinds that never occur back to back: {missing}"
    # ... and no pair occurs that the table calls impossible (the two descriptions of the state machine agree)
    for id_, name, n, ops, _ in ALL:
        for (a, b) in cs.pair_table([ops]):
            assert cs.pair_allowed(cs.SPECS[name], a, b), (id_, a, b)
    unseen = [(k, v) for k, vals in cs.OPTION_VALUES.items() for v in vals if (k, v) not in option_seen]
    assert not unseen, f"option values never followed by a weighted step before the option changes again: {unseen}"
    assert grows >= 20 and shrinks >= 20 and longest_last >= 5, (grows, shrinks, longest_last)


def test_every_model_and_size_of_the_plan_is_there():
    have = {(name, n) for _, name, n, _, _ in ALL}
    for name in ("c1", "c2", "c3", "linear", "c4p1", "c4p2", "rtc"):
        assert any(h[0] == name for h in have), name
    assert any(h[0] in ("studentt", "negbin") for h in have)
    for n in (1, 2, 63, 1000, 1025, 5000, 70 * 1024 + 3):
        assert any(h[1] == n for h in have), n
    assert ("c1", (1 << 20) + 77) in have and ("c2", 1 << 20) in have


@pytest.mark.parametrize("case", FAST, ids=[s[0] for s in FAST])
def test_a_carried_oracle_equals_the_fresh_replay(case):
    """The reference side alone, with the oracle in BOTH roles: one OraclePf carried through the whole sequence (the subject) against
    the fresh replay of the live prefix (the expectation).  Bit for bit after every op and at every checkpoint."""
    id_, name, n, ops, _ = case
    subject = cs.CarriedOracle(cs.SPECS[name], n, 20260101)
    r = cs.run_sequence(subject, name, n, 20260101, ops)
    assert r.ref.particle_steps <= cs.replay_cost(name, n, ops), "the budget below counts at least what the runner spends"


def test_the_runner_notices_a_wrong_subject():
    """The runner against a subject that is wrong in one carried field: it must name the op."""
    class KeepsItsKey(cs.CarriedOracle):
        def reseed(self, seed):          # the new key does not reach the filter
            self.seed = int(seed)
    seq = [op("init", 0.0), op("step", 1.0, 2.0, 1), op("reseed", 99), op("step", 2.0, 1.0, 1), op("particles")]
    with pytest.raises(cs.Divergence) as e:
        cs.run_sequence(KeepsItsKey(cs.SPECS["c2"], 500, 7), "c2", 500, 7, seq)
    assert "op 3 op('step', 2.0, 1.0, 1)" in str(e.value) and "op('reseed', 99)" in str(e.value)

    class ForgetsTheAdoptedEss(cs.CarriedOracle):
        def adopt(self, cloud, ll, ess):
            super().adopt(cloud, ll, ess + 1)
    seq = [op("init", 0.0), op("propagate", 1.0, 2.0, 1), op("adopt", 0.3125), op("step", 2.0, 0.0, 0)]
    with pytest.raises(cs.Divergence, match="ess differs"):
        cs.run_sequence(ForgetsTheAdoptedEss(cs.SPECS["c1"], 300, 7), "c1", 300, 7, seq)


def test_budget_of_the_gpu_sequences():
    """Oracle time, from the oracle's measured speed (0.50 us per particle-step at d = 1, 0.67 at d = 3, 1.2 at d = 9; one thread):
    the non-slow sequences together stay under 6e7 particle-steps of fresh replay, replays at checkpoints included."""
    from test_gpu_call_sequences import HAND      # (the hand-written sequences of the GPU half count too, and are legal)
    for spec_name, n, ops in HAND.values():
        cs.check_legal(cs.SPECS[spec_name], ops)
    total = sum(cs.replay_cost(name, n, ops) for _, name, n, ops, _ in FAST) + sum(cs.replay_cost(*h) for h in HAND.values())
    assert 0 < total <= cs.BUDGET, f"{total:.3g} particle-steps"
    for _, name, n, ops, slow in ALL:
        if slow:
            assert len(ops) <= 16
