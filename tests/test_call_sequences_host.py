"""The CPU half of the call-sequence tests (tests/call_sequences.py; the GPU half is tests/test_gpu_call_sequences.py).

Nothing here needs a GPU: the generator is deterministic and emits only sequences the documented state machine allows; the
committed seed list covers the vocabulary (a condition the test computes, not a hope); the reference side is sound -- ONE oracle
object carried through a whole sequence equals the fresh replay of its live prefix after every op, bit for bit, so the expectation
the GPU half compares with has no stale state of its own; and the oracle time of the non-slow GPU sequences stays within a budget
that is counted from the sequences themselves."""
from __future__ import annotations

import hashlib

import numpy as np
import pytest

import call_sequences as cs
from call_sequences import op

ALL = cs.committed_sequences()
FAST = [s for s in ALL if not s[4]]
ALL_V2 = cs.committed_sequences_v2()
FAST_V2 = [s for s in ALL_V2 if not s[4]]
# SHA-256 over id + pasteable(ops) of every entry of committed_sequences(), computed before the second vocabulary was added
V1_DIGEST = "de961f0909e4b0a0e1aa5847cd07c8d88d2645e17e8dbf0ecbece690edd7e213"


def test_the_first_vocabulary_s_committed_sequences_have_not_moved():
    """sequence(), SEQUENCES, SLOW_SEQUENCES, STATE_KINDS, pair_allowed, pair_snippet, committed_sequences() produce, op for op, what
    they produced before the V2 layer was written (the seeded generator draws from one random.Random: a new branch would move all)."""
    h = hashlib.sha256()
    for id_, _, _, ops, _ in ALL:
        h.update((id_ + cs.pasteable(ops)).encode())
    assert h.hexdigest() == V1_DIGEST and len(ALL) == 43
    assert cs.BUDGET == 6e7 and len(cs.STATE_KINDS) == 17 and cs.STATE_KINDS_V2[:17] == cs.STATE_KINDS


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


@pytest.mark.parametrize("case", FAST + FAST_V2, ids=[s[0] for s in FAST + FAST_V2])
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

    class KeysFromTheSeedBeforeTheReseed(cs.CarriedOracle):
        def reseed(self, seed):          # the filter takes the new key, the default forecast keys keep the old one
            self.o.reseed(int(seed))
    seq = [op("init", 0.0), op("step", 1.0, 2.0, 1), op("reseed", 99), op("run_forecasts_more", 3, 5, 0, 0.975, None), op("particles")]
    with pytest.raises(cs.Divergence) as e:
        cs.run_sequence(KeysFromTheSeedBeforeTheReseed(cs.SPECS["c2"], 500, 7), "c2", 500, 7, seq)
    assert "op 3 op('run_forecasts_more', 3, 5, 0, 0.975, None)" in str(e.value) and "forecast keys differ" in str(e.value)

    class SummarisesBeforeTheStep(cs.CarriedOracle):
        def step_intervals(self, t, y, has, interval):
            row = self.o.summary(interval)
            return self.step(t, y, has) + row
    seq = [op("init", 0.0), op("step", 1.0, 2.0, 1), op("step_intervals", 2.0, 1.0, 1, 0.9), op("particles")]
    with pytest.raises(cs.Divergence) as e:
        cs.run_sequence(SummarisesBeforeTheStep(cs.SPECS["c2"], 500, 7), "c2", 500, 7, seq)
    assert "op 2 op('step_intervals', 2.0, 1.0, 1, 0.9)" in str(e.value) and "step_intervals row" in str(e.value)


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


# ----------------------------------------------------------------------------- the second vocabulary
def test_v2_generator_is_deterministic_and_every_sequence_is_legal():
    for seed, name, n, length, mt in cs.SEQUENCES_V2 + cs.SLOW_SEQUENCES_V2:
        a, b = cs.sequence_v2(seed, name, n, length, mt), cs.sequence_v2(seed, name, n, length, mt)
        assert a == b and repr(a) == repr(b)
        assert len(a) >= length
        assert eval(cs.pasteable(a), {"op": op}) == a, "a printed sequence pastes back into the same ops"
    assert cs.sequence_v2(1, "c2", 1000, 30) != cs.sequence_v2(2, "c2", 1000, 30)
    for id_, name, n, ops, _ in ALL_V2:
        st = cs.check_legal(cs.SPECS[name], ops)
        assert st.usable() and not st.cloud_unknown, id_
        for o in ops:                     # the sizes the generator keeps for the slowest expectations
            if o.kind == "smooth":
                assert n <= 5000 and o[3] <= 64 and o[1] <= 12, (id_, o)
            if o.kind == "pmmh":
                assert n <= 5000 and o[3] <= 4 and o[1] <= 6, (id_, o)
    for name in ("c1", "c2", "c3", "linear", "c4p1", "rtc"):
        assert any(s[1] == name for s in ALL_V2), name
    assert any(s[1] in ("studentt", "negbin") for s in ALL_V2)
    for n in (1, 2, 63, 512, 513, 1000, 4097, 5000, 70 * 1024 + 3):
        assert any(s[2] == n and not s[4] for s in ALL_V2), n
    big = [s for s in ALL_V2 if s[2] == 131073]
    assert len(big) == 1 and big[0][1] == "c2" and not big[0][4] and len(big[0][3]) <= 14
    assert all(o[1] <= 4 for o in big[0][3] if o.kind in cs.BATCH_ROWS + ("run", "run_more"))
    slow = [s for s in ALL_V2 if s[4]]
    assert [(s[1], s[2]) for s in slow] == [("c1", 300001)] and len(slow[0][3]) <= 12
    assert all(o[1] <= 3 for o in slow[0][3] if o.kind in cs.BATCH_ROWS + ("run", "run_more"))


def test_the_state_machine_refuses_what_the_header_refuses_of_the_v2_calls():
    c2, lg = cs.SPECS["c2"], cs.SPECS["c4p1"]
    pm = [op("init", 0.0), op("pmmh", 3, 1, 2, 0.01, 5)]
    for spec, bad in ((c2, [op("run_intervals_more", 2, 1, 0.9, None)]),                      # continuing calls before init
                      (c2, [op("step_forecast", 1.0, 1.0, 1, None, 0.9)]),
                      (c2, [op("run_intervals", 0, 1, 0.9, None)]),                           # empty data
                      (c2, [op("run_forecasts", 3, 1, 0, 1.5, None)]),                        # an interval outside (0, 1]
                      (c2, [op("init", 2.0), op("step_intervals", 1.0, 1.0, 1, 0.9)]),        # time before the clock
                      (c2, [op("smooth", 3, 1, 8, 0.9), op("step_intervals", 9.0, 1.0, 1, 0.9)]),   # the handle must be re-initialised
                      (c2, [op("smooth", 3, 1, 0, 0.9)]),
                      (c2, pm + [op("init", 0.0)]),                                           # parameters and key unknown behind pmmh
                      (c2, pm + [op("set_params", 1), op("init", 0.0)]),
                      (c2, pm + [op("reseed", 1), op("run_intervals", 3, 1, 0.9, None)]),
                      (c2, pm + [op("set_params", 1), op("reseed", 1), op("step", 9.0, 1.0, 1)]),   # ... and then a NEW cloud
                      (c2, pm + [op("particles")]),
                      (c2, pm + [op("forecast_key")]),
                      (c2, [op("init", 0.0), op("set_option", 2, 1), op("run_forecasts_more", 2, 1, 0, 0.9, None)]),
                      (c2, [op("init", 0.0), op("refused", "EINVAL_ARG", op("step_intervals", 1.0, 1.0, 1, 0.9))]),   # ... it would be accepted
                      (c2, [op("init", 0.0), op("refused", "ESTATE", op("run_intervals_more", 2, 1, 0.9, None))]),
                      (c2, [op("refused", "EINVAL_ARG", op("run_intervals_more", 0, 1, 0.9, None))]),                 # ESTATE comes first
                      (lg, [op("run_forecasts", 3, 1, 0, 0.9, None)]), (lg, [op("smooth", 3, 1, 8, 0.9)]),
                      (lg, [op("run_intervals", 3, 1, 0.9, 1)]),                              # no datum to replace
                      (lg, [op("init", 0.0), op("fails", "ENONFINITE", op("step_intervals", -1.0, 1.0, 1, 0.9))])):
        with pytest.raises(cs.IllegalSequence):
            cs.check_legal(spec, bad)
    cs.check_legal(c2, pm + [op("refused", "EINVAL_ARG", op("smooth_pairing", 3, 1, 8, 0.9)), op("set_option", 6, 1), op("reseed", 1), op("set_params", 2),
                             op("run_forecasts", 3, 1, 0, 0.9, None), op("forecast_key"), op("observation_index")])
    cs.check_legal(lg, [op("run_intervals", 3, 1, 0.9, None), op("refused", "EINVAL_ARG", op("step_forecast", 9.0, 1.0, 1, None, 0.9)), op("pmmh", 2, 1, 1, 0.01, 3)])


def _refusal_class(spec, o):
    """The documented refusal an op("refused", ...) of the V2 calls stands for."""
    code, inner = o[1], o[2]
    ik = inner.kind
    if code == "ESTATE":
        return f"refused:ESTATE:{ik}"
    if ik == "smooth_pairing":
        return "refused:EINVAL_ARG:smooth_reference_pairing"
    if ik in cs.BATCH_ROWS and inner[1] == 0:
        return "refused:EINVAL_ARG:T0"
    iv = cs.interval_of(inner)
    if iv is not None and not 0.0 < iv <= 1.0:
        return f"refused:EINVAL_ARG:interval_{iv}"
    if ik == "smooth" and inner[3] == 0:
        return "refused:EINVAL_ARG:smooth_M0"
    assert spec.lgcp, o
    return "refused:EINVAL_ARG:lgcp_smooth" if ik == "smooth" else "refused:EINVAL_ARG:lgcp_" + ik


REQUIRED_V2 = (cs.NEW_KINDS + tuple(f"refused:ESTATE:{k}" for k in cs.CONTINUING) +
               ("refused:EINVAL_ARG:T0", "refused:EINVAL_ARG:interval_0.0", "refused:EINVAL_ARG:interval_1.5", "refused:EINVAL_ARG:smooth_M0",
                "refused:EINVAL_ARG:smooth_reference_pairing", "refused:EINVAL_ARG:lgcp_smooth", "refused:EINVAL_ARG:lgcp_forecasts",
                "fails:step_intervals", "fails:step_forecast", "outlier_at", "keyed0", "keyed1", "rows_missing_datum", "rows_dt0",
                "interval_0.975", "interval_0.9", "interval_1.0", "interval_rank_clamps"))


def test_coverage_of_the_committed_v2_sequences():
    """Every V2 kind, refusal and failure at least 5 times; outliers, both key modes, records without a datum and dt = 0 inside rows calls at
    least 5 times; every ordered pair with a V2 kind in it that pair_allowed_v2 allows at least once and none it forbids; every option value
    followed by a V2 weighted kind before that option changes again; a rows call of more than 1024 records behind a shorter one at least 3
    times at N <= 1000; a shorter smooth behind a longer one at least twice."""
    counts = {}

    def bump(k):
        counts[k] = counts.get(k, 0) + 1
    option_seen = set()
    long_behind_short = shorter_smooth = 0
    for id_, name, n, ops, _ in ALL_V2:
        spec = cs.SPECS[name]
        st = cs.HostState(spec)
        waiting = {}
        rows_T, smooth_T = [], []
        for o in ops:
            k = o.kind
            if k == "refused" and (o[2].kind in cs.NEW_KINDS or o[2].kind == "smooth_pairing"):
                c = _refusal_class(spec, o)
                bump(c)
                if c.startswith("refused:EINVAL_ARG:lgcp_") and o[2].kind in cs.FORECAST_KINDS:
                    bump("refused:EINVAL_ARG:lgcp_forecasts")
            elif k == "fails":
                bump("fails:" + o[2].kind)
            elif k in cs.NEW_KINDS:
                bump(k)
                iv = cs.interval_of(o)
                if iv is not None:
                    bump("interval_rank_clamps" if int(np.floor(iv * n)) == 0 else f"interval_{iv}")
            if k in cs.BATCH_ROWS:
                t, y, has = cs.data_of(spec, o, st.t)
                if cs.outlier_at(o) is not None:
                    assert y[cs.outlier_at(o)] == spec.outlier and has[cs.outlier_at(o)]
                    bump("outlier_at")
                if k in cs.FORECAST_KINDS:
                    bump(f"keyed{o[3]}")
                if not has.all():
                    bump("rows_missing_datum")
                prev = np.concatenate(([st.t], t[:-1]))
                if np.any((t == prev)[(0 if k in cs.CONTINUING else 1):]):
                    bump("rows_dt0")
                if o[1] > 1024 and n <= 1000 and rows_T and min(rows_T) < o[1]:
                    long_behind_short += 1
                rows_T.append(o[1])
            if k == "smooth":
                shorter_smooth += bool(smooth_T and o[1] < max(smooth_T))
                smooth_T.append(o[1])
            if k == "set_option" and o[1] in cs.OPTION_VALUES:
                waiting[o[1]] = o[2]
            elif k in cs.NEW_KINDS and cs.is_weighted_op(spec, st, o):
                option_seen.update(waiting.items())
                waiting.clear()
            elif cs.is_weighted_op(spec, st, o):
                waiting.clear()           # (a weighted step of the first vocabulary took the option's first use)
            st.apply(o)
    few = {k: counts.get(k, 0) for k in REQUIRED_V2 if counts.get(k, 0) < 5}
    assert not few, f"V2 kinds, refusals and variants that occur fewer than 5 times: {few}"
    tab = cs.pair_table_v2([s[3] for s in ALL_V2])
    spec = cs.SPECS[cs.COMPLETION[0]]
    new = cs.NEW_KINDS
    missing = [(a, b) for a in cs.STATE_KINDS_V2 for b in cs.STATE_KINDS_V2
               if (a in new or b in new) and cs.pair_allowed_v2(spec, a, b) and (a, b) not in tab]
    assert not missing, f"ordered pairs with a V2 kind that never occur back to back: {missing}"
    for id_, name, n, ops, _ in ALL_V2:
        for (a, b) in cs.pair_table([ops]):
            assert cs.pair_allowed_v2(cs.SPECS[name], a, b), (id_, a, b)
    for a in cs.STATE_KINDS:              # on the first vocabulary the two tables are one
        for b in cs.STATE_KINDS:
            assert cs.pair_allowed_v2(spec, a, b) == cs.pair_allowed(spec, a, b)
    unseen = [(k, v) for k, vals in cs.OPTION_VALUES.items() for v in vals if (k, v) not in option_seen]
    assert not unseen, f"option values never followed by a V2 weighted kind before the option changes again: {unseen}"
    assert long_behind_short >= 3 and shorter_smooth >= 2, (long_behind_short, shorter_smooth)
    for id_, name, n, ops, _ in ALL_V2:  # each completion snippet ends with a weighted step and a look at the cloud
        if id_.startswith("vpairs"):
            ends = [i for i, o in enumerate(ops) if o.kind == "particles"]
            assert ends and ends[-1] == len(ops) - 1
            assert all(ops[i - 1].kind in ("step", "step_intervals") and ops[i - 1][3] for i in ends), id_
            assert name == cs.COMPLETION[0] and n == cs.COMPLETION[1]


def test_budget_of_the_v2_gpu_sequences():
    """The V2 non-slow list and the hand-written V2 sequences together stay within cs.BUDGET on their own account; replay_cost counts the
    forecast expectations (FORECAST_ROW_COST particle-steps per particle and row: a new oracle of the cloud, one transition) and the
    smoother's twin (its M x N backward weights per record, SMOOTH_TWIN_PER_STEP of them to a particle-step)."""
    from test_gpu_call_sequences_v2 import HAND_V2
    for spec_name, n, ops in HAND_V2.values():
        cs.check_legal(cs.SPECS[spec_name], ops)
    total = sum(cs.replay_cost(name, n, ops) for _, name, n, ops, _ in FAST_V2) + sum(cs.replay_cost(*h) for h in HAND_V2.values())
    assert 0 < total <= cs.BUDGET, f"{total:.3g} particle-steps"
    n, T, M = 5000, 12, 64
    plain = cs.replay_cost("c2", n, [op("run_intervals", T, 1, 0.9, None)], checkpoints=False)
    assert cs.replay_cost("c2", n, [op("run_forecasts", T, 1, 0, 0.9, None)], checkpoints=False) == plain + cs.FORECAST_ROW_COST * n * T
    assert cs.replay_cost("c2", n, [op("smooth", T, 1, M, 0.9)], checkpoints=False) == 2 * plain + M * n * T // cs.SMOOTH_TWIN_PER_STEP
    assert cs.replay_cost("c2", n, [op("pmmh", 6, 1, 4, 0.01, 3)], checkpoints=False) == 4 * (6 + 1) * n
