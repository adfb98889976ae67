"""Model-based testing of REUSED filter handles: seeded sequences of public calls on ONE handle, the expected result of every
call computed from a FRESH oracle that replays the live prefix, compared bit for bit.

A handle (csrc/cssm_internal.h: cssm_pf) carries a lot of host-side state from one call to the next -- which buffer holds the cloud
and in which layout, whether the ancestors are valid, whether `logw` holds weights or log-weights, the max-slot set of the next
weighted step, which sums the last propagate left, the predicted reference level, capacities that only grow -- and
cssm_pf_set_option changes the launch geometry at any moment.  PMMH, the streaming Filter and the batch handle all live on
reused handles; this module drives them the same way.

  op(kind, *args)          one call, printed as a line of Python (a failing sequence can be pasted into a test)
  HostState                the documented state machine of a handle in pure Python: legality of a sequence, clock, observation count
  sequence(seed, ...)      the seeded generator; committed_sequences() = the committed list, completed deterministically so that the
                           coverage conditions of tests/test_call_sequences_host.py hold
  Ref                      the expectation: a NEW oracle.OraclePf replaying the live prefix (cached between ops, rebuilt from scratch at
                           every checkpoint, the rebuilt one compared with the cached one)
  run_sequence(subject,..) the runner; `subject` is a NativePf (GPU) or a CarriedOracle (one oracle object carried through the whole
                           sequence: the check that the expectation itself has no stale state, which runs without a GPU)

The SECOND vocabulary (V2: STATE_KINDS_V2, sequence_v2, SEQUENCES_V2, committed_sequences_v2) adds the calls that came behind the first:
the rows calls (cssm_pf_filter_intervals / _more / cssm_pf_step_intervals, cssm_pf_filter_forecasts / _more / cssm_pf_step_forecast),
cssm_pf_smooth and cssm_pmmh_run on THIS handle.  The first vocabulary -- sequence(), SEQUENCES, pair_allowed, pair_snippet,
committed_sequences() -- produces op for op what it produced before (tests/test_call_sequences_host.py holds a digest of it); the V2
generator draws from a random.Random of its own.  Expectations, all from the fresh-replay oracle: interval rows = the oracle's init;
summary; (step; summary)* with the means formed exactly (summary_row); forecast row s = test_gpu_forecast.expected from the oracle's cloud
BEFORE record s under the key the reference derives; smooth = smooth_expected; pmmh = OraclePf.pmmh.
pmmh is used on EVERY spec of SPECS: cssm_pmmh_run is set_params + reseed + cssm_pf_filter per iteration on the handle as it stands (its
resampler option, its LGCP precision, a run-time-compiled structure included), and oracle_pmmh_run is the same loop over oracle_pf_filter
under the resampler flag the oracle was created with -- neither refuses a structure the filter serves.  The header promises nothing about
the parameters and the key cssm_pmmh_run leaves: behind it only set_params, reseed, set_option and refused calls are legal until a
set_params and a reseed have both followed, and then a call that draws a new cloud (HostState.cloud_unknown, the shape of
resampler_pending).  smooth and pmmh stay at N <= 5000 (M <= 64, T <= 12; iters <= 4, T <= 6): their expectations are the slowest.

Plain module: no fixtures, no test functions.
"""
from __future__ import annotations

import math
import random
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

import cases
from composablestatespacemodels_amd.model import Model, Parameters, UnparamModel
from oracle import oracle

# ---- status codes (include/cssm_pf.h)
EINVAL_DESC, EHIP, ENONFINITE, EINVAL_ARG, ESTATE = -1, -2, -5, -6, -7
CODES = {"EINVAL_DESC": EINVAL_DESC, "ENONFINITE": ENONFINITE, "EINVAL_ARG": EINVAL_ARG, "ESTATE": ESTATE}

# ---- options (include/cssm_pf.h) and their documented values
OPT_EXACT, OPT_RESAMPLER, OPT_FUSED, OPT_WHOLE, OPT_GROUP, OPT_SPECIALISE, OPT_WAVE, OPT_FORECAST_CAP = 1, 2, 3, 6, 7, 8, 10, 11
OPTION_VALUES = {OPT_EXACT: (0, 1, 2), OPT_RESAMPLER: (0, 1, 2), OPT_FUSED: (0, 1), OPT_WHOLE: (0, 1, 2, 3), OPT_GROUP: (0, 1),
                 OPT_SPECIALISE: (0, 1, 2), OPT_WAVE: (0, 1, 2)}
OPTION_DEFAULTS = {OPT_EXACT: 0, OPT_RESAMPLER: 0, OPT_FUSED: 1, OPT_WHOLE: 0, OPT_GROUP: 1, OPT_SPECIALISE: 1, OPT_WAVE: 1}
RESAMPLER_FLAGS = {0: 0, 1: oracle.RESAMPLE_STRATIFIED, 2: oracle.RESAMPLE_MULTINOMIAL}


class Op(tuple):
    """(kind, *args); repr is the line of Python that makes it."""

    def __new__(cls, kind, *args):
        return super().__new__(cls, (kind,) + args)

    kind = property(lambda self: self[0])
    args = property(lambda self: tuple(self[1:]))

    def __repr__(self):
        return "op(" + ", ".join(repr(a) for a in self) + ")"


def op(kind, *args) -> Op:
    return Op(kind, *args)


def pasteable(seq: Sequence[Op]) -> str:
    return "[\n" + "".join(f"    {o!r},\n" for o in seq) + "]"


# Kinds.  State-changing ones are what the coverage table pairs up (set_option per option: "opt3").
RESTARTS = ("init", "init_from", "run", "interpolate")
STATE_KINDS = ("init", "init_from", "step", "propagate", "adopt", "run", "run_more", "set_params", "reseed", "interpolate") + \
    tuple(f"opt{k}" for k in OPTION_VALUES)
READ_KINDS = ("summary", "forecast", "forecast_posterior", "particles", "proposed", "weights", "logw", "ancestors", "observation_index",
              "forecast_key", "last_device_us")
ILLEGAL_KINDS = ("refused", "fails")
# variants of `step` the generator must produce (counted as kinds of their own in the coverage table)
STEP_VARIANTS = ("step_missing", "step_dt0", "step_outlier")


# ---- the second vocabulary (V2): the calls that form rows inside the filtering call, the smoother, and PMMH on a handle that lives on.
# The first vocabulary above stays as it is; sequence() never emits one of these.
#   run_intervals(T, dseed, interval, outlier_at)           cssm_pf_filter_intervals         draws a new cloud (every spec)
#   run_intervals_more(T, dseed, interval, outlier_at)      cssm_pf_filter_intervals_more    continues
#   step_intervals(t, y, has, interval)                     cssm_pf_step_intervals           one step
#   run_forecasts(T, dseed, keyed, interval, outlier_at)    cssm_pf_filter_forecasts         draws a new cloud (not LGCP)
#   run_forecasts_more(T, dseed, keyed, interval, outlier_at)  cssm_pf_filter_forecasts_more continues (not LGCP)
#   step_forecast(t, y, has, key or None, interval)         cssm_pf_step_forecast            one step (not LGCP)
#   smooth(T, dseed, M, interval)                           cssm_pf_smooth                   like interpolate: re-initialise afterwards (not LGCP)
#   pmmh(T, dseed, iters, delta, seed)                      cssm_pmmh_run on THIS handle     leaves parameters, key and cloud unknown
INTERVAL_KINDS = ("run_intervals", "run_intervals_more", "step_intervals")
FORECAST_KINDS = ("run_forecasts", "run_forecasts_more", "step_forecast")
ROW_KINDS = INTERVAL_KINDS + FORECAST_KINDS
NEW_KINDS = ROW_KINDS + ("smooth", "pmmh")
STATE_KINDS_V2 = STATE_KINDS + NEW_KINDS
NEW_RESTARTS = ("run_intervals", "run_forecasts", "smooth", "pmmh")
ALL_RESTARTS = RESTARTS + NEW_RESTARTS
BATCH_ROWS = ("run_intervals", "run_intervals_more", "run_forecasts", "run_forecasts_more")
CONTINUING = ("run_intervals_more", "step_intervals", "run_forecasts_more", "step_forecast")   # need a running filter
STEP_ROWS = ("step_intervals", "step_forecast")
SMOOTH_MAX_M = 4096              # CSSM_FLEET_MAX_N


def state_kind(o: Op) -> Optional[str]:
    """The state-changing kind of an op for the pair table, None for read-only and refused calls."""
    if o.kind == "set_option":
        return f"opt{o[1]}" if o[1] in OPTION_VALUES else None
    return o.kind if o.kind in STATE_KINDS_V2 else None


def interval_of(o: Op) -> Optional[float]:
    """The interval argument of a V2 op (None: the kind has none)."""
    k = o.kind
    if k in ("run_intervals", "run_intervals_more"):
        return o[3]
    if k in ("step_intervals", "run_forecasts", "run_forecasts_more", "smooth", "smooth_pairing"):
        return o[4]
    if k == "step_forecast":
        return o[5]
    return None


def outlier_at(o: Op) -> Optional[int]:
    k = o.kind
    if k in ("run_intervals", "run_intervals_more"):
        return o[4]
    if k in ("run_forecasts", "run_forecasts_more"):
        return o[5]
    return None


def _bad_interval(v) -> bool:
    return not (0.0 < v <= 1.0)


# --------------------------------------------------------------------------------------------- models and data
class Spec:
    """A model of the sequences: factory, LGCP precision, the data its observations are drawn like, a second structure for the
    refused set_params."""

    def __init__(self, name, make, data, precision=0, outlier=400.0):
        self.name, self.make, self.data, self.precision, self.outlier = name, make, data, precision, outlier
        self._base = None

    @property
    def lgcp(self):
        return self.data == "lgcp"

    def model(self, k: int = 0) -> Model:
        """Parameter variant k of the model: same structure, every stored parameter moved (k = 0: the model itself)."""
        if self._base is None:
            self._base = self.make()
        if k == 0:
            return self._base
        um = UnparamModel([spec for spec, _, _ in self._base.leaves])
        p0 = Parameters([node for _, node, _ in self._base.leaves])
        th = np.asarray(p0.flattenParams())
        return um.run(p0.withFlat(th + 0.04 * k * np.cos(np.arange(th.size) + k)))

    def other_structure(self) -> Model:
        """A model of another latent dimension: what cssm_pf_set_params refuses."""
        return cases.c2_model() if self.dim() == 1 else cases.c1_model()

    def dim(self) -> int:
        return sum(sde.dimension for _, _, sde in self.model().leaves)


def _outside_the_table():
    from test_gpu_rtc import outside_the_table
    return outside_the_table()


SPECS: Dict[str, Spec] = {s.name: s for s in (
    Spec("c1", cases.c1_model, "poisson"),
    Spec("c2", cases.c2_model, "poisson"),
    Spec("c3", cases.c3_model, "poisson"),
    Spec("linear", cases.linear_model, "gaussian", outlier=60.0),
    Spec("studentt", cases.studentt_model, "gaussian", outlier=1.0e6),
    Spec("negbin", cases.negbin_model, "poisson"),
    Spec("c4p1", cases.c4_model, "lgcp", precision=1),
    Spec("c4p2", cases.c4_model, "lgcp", precision=2),
    Spec("rtc", _outside_the_table, "poisson"),
)}

_DTS = (0.0, 0.25, 0.5, 1.0, 1.0, 1.5)          # exactly representable increments; dt = 0 included
_DTS_LGCP = (0.0, 0.125, 0.25, 0.25)


def series(spec: Spec, T: int, dseed: int, t_start: float, continuing: bool):
    """(t, y, has) of T observations, a function of (spec.data, T, dseed, t_start) alone.  A new series starts AT t_start (its first
    increment is 0, as llFilter's t0 = min t makes it); a continued one goes on behind t_start."""
    rng = np.random.default_rng([int(dseed), int(T), 77])
    dt = rng.choice(_DTS_LGCP if spec.lgcp else _DTS, size=T)
    if T and not continuing:
        dt[0] = 0.0
    t = t_start + np.cumsum(dt)
    if spec.data == "poisson":
        y = rng.poisson(2.0, T).astype(np.float64)
    elif spec.data == "gaussian":
        y = 0.5 + rng.standard_normal(T)
    else:
        y = np.ones(T)
    has = np.ones(T, dtype=np.uint8) if spec.lgcp else (rng.random(T) >= 0.2).astype(np.uint8)
    if T and not spec.lgcp and not continuing:
        has[0] = 1                       # (a continued series may well start on a missing observation)
    return t, y, has


def data_of(spec: Spec, o: Op, clock: float):
    """(t, y, has) of a batch op of either vocabulary: series() of its (T, dseed), continued behind `clock` for the *_more kinds, a new
    series otherwise; the record at outlier_at takes spec.outlier as its datum (its level is ruled out by the max: held and redone)."""
    cont = o.kind in ("run_more", "run_intervals_more", "run_forecasts_more")
    t, y, has = series(spec, o[1], o[2], clock if cont else float(o[2] % 3), cont)
    at = outlier_at(o)
    if at is not None:
        y, has = y.copy(), has.copy()
        y[at], has[at] = spec.outlier, 1
    return t, y, has


def row_keys(dseed: int, T: int) -> np.ndarray:
    """The given keys of a forecast call with keyed = 1: a function of (dseed, record) alone."""
    return np.array([int(oracle.lib().oracle_c_derive_key(0xF0CA57 + int(dseed), s + 1)) for s in range(T)], dtype=np.uint64)


def theta_of(model: Model) -> np.ndarray:
    return np.asarray(Parameters([node for _, node, _ in model.leaves]).flattenParams(), dtype=np.float64)


def substeps(spec: Spec, dt: float) -> int:
    """Transitions per particle of one observation (LGCP: FilterLgcp's sub-steps) -- the unit of the oracle-time budget."""
    if not spec.lgcp:
        return 1
    return max(1, int(math.ceil(dt / 10.0 ** -spec.precision)))


def horizon_times(t0: float, H: int) -> np.ndarray:
    return t0 + np.cumsum(np.array([0.5, 0.0, 1.25, 1.25, 4.25])[:H])


# --------------------------------------------------------------------------------------------- the documented state machine
class IllegalSequence(AssertionError):
    pass


class HostState:
    """What include/cssm_pf.h lets a caller know about a handle: initialised or not, failed mid-series, the clock, the observation
    count, whether a weighted step has run since the cloud was drawn, whether a weighted propagate awaits its adopt, the options."""

    def __init__(self, spec: Spec):
        self.spec = spec
        self.initialised = False
        self.failed = False
        self.t = 0.0
        self.obs = 0
        self.weighted = False           # a weighted step since the cloud was drawn: weights()/logw() are defined
        self.pending_adopt = False
        self.resampler_pending = False  # option 2 changed: the next state change must draw a new cloud
        self.after_run_more = False
        # V2: cssm_pmmh_run re-parameterises and reseeds the handle every iteration and promises nothing about what it leaves
        self.cloud_unknown = self.params_unknown = self.seed_unknown = False
        self.opts = dict(OPTION_DEFAULTS)
        self.model_k = 0
        self.last_state_kind: Optional[str] = None
        self.last_cloud_kind: Optional[str] = None    # the last call that touched the cloud (options, parameters and keys do not)

    def usable(self) -> bool:
        return self.initialised and not self.failed

    # -- what may come next
    def legal(self, o: Op) -> Optional[str]:
        """None if `o` is legal now, else the reason."""
        k = o.kind
        if self.resampler_pending and k not in ALL_RESTARTS + ("set_option", "set_params", "reseed", "refused"):
            return "after a change of the resampler only a call that draws a new cloud may follow"
        if self.cloud_unknown:
            if k in ALL_RESTARTS:
                if self.params_unknown or self.seed_unknown:
                    return "after pmmh the parameters and the key are unknown until a set_params and a reseed have both followed"
            elif k not in ("set_option", "set_params", "reseed", "refused"):
                return "after pmmh only set_params, reseed, set_option and refused calls may come before a new cloud"
        if k == "refused":
            code, inner = o[1], o[2]
            ik = inner.kind
            if code == "ESTATE" and ik in ("step", "run_more", "summary", "propagate"):
                return None if not self.initialised else "refused(ESTATE) needs an uninitialised handle"
            if code == "EINVAL_ARG" and ik == "set_option" and inner[1] == OPT_RESAMPLER and inner[2] not in OPTION_VALUES[OPT_RESAMPLER]:
                return None
            if code == "EINVAL_ARG" and ik in ("run", "run_more") and inner[1] == 0:
                return None
            if code == "EINVAL_DESC" and ik == "set_params_other":
                return None
            if ik in NEW_KINDS or ik == "smooth_pairing":
                return self._refusal_v2(code, inner)
            return "no documented refusal of this call"
        if k == "fails":
            inner = o[2]
            if o[1] != "ENONFINITE" or inner.kind not in ("step",) + STEP_ROWS or self.spec.lgcp:
                return "only a weighted step back in time is a documented mid-series failure (not LGCP: its sub-step count is dt / delta)"
            if not self.usable() or not (inner[1] < self.t) or not inner[3]:
                return "a failing step needs a running filter, a time before the clock and an observation"
            return None
        if k in ("init", "init_from", "set_params", "reseed"):
            return None
        if k == "set_option":
            if o[1] == OPT_FORECAST_CAP:
                return None if o[2] >= 0 else "cap < 0"
            if o[1] not in OPTION_VALUES or o[2] not in OPTION_VALUES[o[1]]:
                return "undocumented option value"
            return None
        if k in ("run", "interpolate"):
            if o[1] < 1:
                return "empty data is refused"
            if k == "interpolate" and self.spec.lgcp:
                return "FilterInterpolate has no LGCP variant"
            return None
        if k in ("step", "propagate"):
            if not self.usable():
                return "needs a running filter"
            return None if o[1] >= self.t else "time before the clock"
        if k == "run_more":
            if not self.usable():
                return "needs a running filter"
            return None if o[1] >= 1 else "empty data is refused"
        if k == "adopt":
            return None if self.usable() and self.pending_adopt else "adopt follows a weighted propagate"
        if k in ("weights", "logw"):
            return None if self.usable() and self.weighted else "no weighted step since the cloud was drawn"
        if k == "last_device_us":
            return None if self.usable() and self.after_run_more else "asked directly behind run_more"
        if k == "forecast":
            if self.spec.lgcp:
                return "the reference leaves LGCP's observation unimplemented"
            return None if self.usable() else "needs a running filter"
        if k == "forecast_posterior":
            return None if not self.spec.lgcp else "the reference leaves LGCP's observation unimplemented"
        if k in ("summary", "particles", "proposed", "ancestors", "observation_index", "forecast_key"):
            return None if self.usable() else "needs a running filter"
        if k in NEW_KINDS:
            return self._legal_v2(o)
        return f"unknown op kind {k!r}"

    def _legal_v2(self, o: Op) -> Optional[str]:
        k, lg = o.kind, self.spec.lgcp
        if lg and (k in FORECAST_KINDS or k == "smooth"):
            return "the forecast kinds and the smoother do not serve an LGCP handle"
        iv = interval_of(o)
        if iv is not None and _bad_interval(iv):
            return "an interval outside (0, 1] is refused"
        if k in STEP_ROWS:
            if not self.usable():
                return "needs a running filter"
            return None if o[1] >= self.t else "time before the clock"
        if o[1] < 1:
            return "empty data is refused"
        at = outlier_at(o)
        if at is not None and (lg or not 0 <= at < o[1]):
            return "the outlier sits on a record of the call (LGCP has no datum to replace)"
        if k in CONTINUING and not self.usable():
            return "needs a running filter"
        if k == "smooth" and not 1 <= o[3] <= SMOOTH_MAX_M:
            return "n_traj outside [1, CSSM_FLEET_MAX_N]"
        if k == "pmmh" and o[3] < 1:
            return "no iteration"
        return None

    def _refusal_v2(self, code: str, inner: Op) -> Optional[str]:
        """The documented refusals of the V2 calls: CSSM_ESTATE for a continuing call on a handle never initialised; CSSM_EINVAL_ARG for
        T = 0, an interval outside (0, 1], n_traj = 0, CSSM_INTERP_REFERENCE_PAIRING, and what an LGCP handle is not served."""
        ik, lg = inner.kind, self.spec.lgcp
        if self.resampler_pending:
            return "between a change of the resampler and the new cloud the reference has no cloud to compare behind a refusal"
        if code == "ESTATE":
            if ik in CONTINUING:
                return None if not self.initialised else "refused(ESTATE) needs an uninitialised handle"
            return "no documented refusal of this call"
        if code != "EINVAL_ARG":
            return "no documented refusal of this call"
        if ik in CONTINUING and not self.usable():
            return "a continuing call is refused with CSSM_ESTATE first where no filter runs"
        if ik in STEP_ROWS and not inner[1] >= self.t:
            return "a step back in time is a failure, not a refusal"
        if ik in ("smooth", "smooth_pairing"):
            if lg or ik == "smooth_pairing" or inner[3] == 0 or _bad_interval(inner[4]):
                return None
            return "the call would be accepted"
        if ik in FORECAST_KINDS and lg:
            return None
        if ik in BATCH_ROWS and inner[1] == 0:
            return None
        if ik in ROW_KINDS and _bad_interval(interval_of(inner)):
            return None
        return "the call would be accepted"

    # -- the state afterwards
    def apply(self, o: Op) -> None:
        why = self.legal(o)
        if why is not None:
            raise IllegalSequence(f"{o!r}: {why}")
        k = o.kind
        sk = state_kind(o)
        if k == "fails":
            self.failed = True
            self.pending_adopt = self.after_run_more = False
            self.last_state_kind = "fails"
            return
        if sk is None:
            return                       # read-only and refused calls leave everything as it was
        self.after_run_more = False
        if k in ("init", "init_from"):
            self._fresh(o[1])
        elif k in ("run", "interpolate"):
            t, _, has = series(self.spec, o[1], o[2], float(o[2] % 3), False)
            self._fresh(float(np.min(t)))
            self.t, self.obs = float(t[-1]), len(t)
            self.weighted = bool(has.any())
            if k == "interpolate":
                self.initialised = False   # "The handle must be re-initialised before further streaming calls."
        elif k == "run_more":
            t, _, has = series(self.spec, o[1], o[2], self.t, True)
            self.t, self.obs = float(t[-1]), self.obs + len(t)
            self.weighted = self.weighted or bool(has.any())
            self.pending_adopt = False
            self.after_run_more = True
        elif k in NEW_RESTARTS:
            t, _, has = data_of(self.spec, o, 0.0)
            self._fresh(float(np.min(t)))
            self.t, self.obs = float(t[-1]), len(t)
            self.weighted = bool(has.any())
            if k == "smooth":
                self.initialised = False   # "The handle must be re-initialised before further streaming calls."
            if k == "pmmh":
                self.cloud_unknown = self.params_unknown = self.seed_unknown = True
        elif k in ("run_intervals_more", "run_forecasts_more"):
            t, _, has = data_of(self.spec, o, self.t)
            self.t, self.obs = float(t[-1]), self.obs + len(t)
            self.weighted = self.weighted or bool(has.any())
            self.pending_adopt = False
        elif k in ("step", "propagate") + STEP_ROWS:
            has = bool(o[3]) or self.spec.lgcp
            self.t, self.obs = float(o[1]), self.obs + 1
            self.weighted = self.weighted or has
            self.pending_adopt = (k == "propagate") and has
        elif k == "adopt":
            self.pending_adopt = False
        elif k == "reseed":
            self.seed_unknown = False
        elif k == "set_params":
            self.model_k = o[1]
            self.params_unknown = False
        elif k == "set_option":
            if o[1] == OPT_RESAMPLER:
                self.resampler_pending = True    # (also where the value stays: one rule for the generator and the pair table)
            self.opts[o[1]] = o[2]
        self.last_state_kind = sk
        if k not in ("set_params", "reseed", "set_option"):
            self.last_cloud_kind = sk

    def _fresh(self, t0):
        self.initialised, self.failed, self.t, self.obs = True, False, float(t0), 0
        self.weighted = self.pending_adopt = self.resampler_pending = False
        self.cloud_unknown = False


def check_legal(spec: Spec, seq: Sequence[Op]) -> HostState:
    st = HostState(spec)
    for i, o in enumerate(seq):
        try:
            st.apply(o)
        except IllegalSequence as e:
            raise IllegalSequence(f"op {i}: {e}\n{pasteable(seq)}") from None
    return st


def is_weighted_op(spec: Spec, st: HostState, o: Op) -> bool:
    """Whether `o` (legal in state `st`) runs at least one weighted observation natively."""
    k = o.kind
    if k == "step":
        return bool(o[3]) or spec.lgcp
    if k == "run":
        return True                      # (the first observation of a new series always carries a datum)
    if k == "run_more":
        return bool(series(spec, o[1], o[2], st.t, True)[2].any())
    if k in STEP_ROWS:
        return bool(o[3]) or spec.lgcp
    if k in NEW_RESTARTS:
        return True
    if k in ("run_intervals_more", "run_forecasts_more"):
        return bool(data_of(spec, o, st.t)[2].any())
    return False


# --------------------------------------------------------------------------------------------- the generator
def _y(spec: Spec, rng: random.Random) -> float:
    if spec.data == "poisson":
        return float(rng.choice((0, 1, 1, 2, 3, 5)))
    if spec.data == "gaussian":
        return rng.choice((-0.75, 0.25, 0.5, 1.5))
    return 1.0


def sequence(seed: int, spec_name: str, n: int, length: int) -> List[Op]:
    """`length` ops on one handle of SPECS[spec_name] with n particles: a function of its arguments alone."""
    spec = SPECS[spec_name]
    rng = random.Random(f"call-sequences/{seed}/{spec_name}/{n}/{length}")
    st = HostState(spec)
    big = n > 20000
    huge = n > 500000
    seq: List[Op] = []
    longest = runs = 0

    def emit(o: Op):
        st.apply(o)
        seq.append(o)

    def run_length():
        nonlocal longest
        if huge:
            T = rng.choice((1, 2, 3))
        elif big:
            T = rng.choice((1, 2, 4, longest + 1 if longest < 6 else 3))
        elif n <= 1000 and rng.random() < 0.2:
            T = 1030 + rng.randrange(40)           # beyond the 1024 records one allocation serves: the buffers regrow
        else:
            T = rng.choice((1, 1, 3, 7, 12, 25, longest + 5 if longest < 40 else 9))
        if spec.precision == 2:
            T = min(T, 6)
        longest = max(longest, T)
        return T

    def next_t():
        return st.t + rng.choice(_DTS_LGCP if spec.lgcp else _DTS)

    def a_step(kind="step"):
        r = rng.random()
        if spec.lgcp:
            return op(kind, next_t(), 1.0, 1)
        if r < 0.15:
            return op(kind, next_t(), 0.0, 0)                         # missing
        if r < 0.25:
            return op(kind, st.t, _y(spec, rng), 1)                   # dt = 0
        if r < 0.37 and kind == "step":
            return op(kind, next_t(), spec.outlier, 1)                # the level is ruled out by the max: redone
        return op(kind, next_t(), _y(spec, rng), 1)

    def an_option():
        k = rng.choice([q for q in OPTION_VALUES if q != OPT_RESAMPLER])
        return op("set_option", k, rng.choice([v for v in OPTION_VALUES[k] if v != st.opts[k]] or list(OPTION_VALUES[k])))

    def a_restart():
        r = rng.random()
        if r < 0.3:
            return op("init", float(rng.choice((0.0, 1.0, 2.5))))
        if r < 0.45:
            return op("init_from", float(rng.choice((0.0, 0.5))), rng.choice((0.0, 0.25, -1.0)))
        if r < 0.9 or spec.lgcp or big:
            nonlocal runs, longest
            runs += 1
            T = run_length()
            if runs == 2 and n <= 1000 and spec.precision != 2:
                T = longest = 1030 + rng.randrange(40)   # every small sequence's second series: the record buffers regrow
            return op("run", T, rng.randrange(1000), int(rng.random() < 0.4))
        return op("interpolate", min(run_length(), 12), rng.randrange(1000), rng.choice((0.975, 0.9)))

    def a_read():
        kinds = ["summary", "particles", "ancestors", "observation_index", "forecast_key", "proposed"]
        if st.weighted:
            kinds += ["weights", "logw"]
        if not spec.lgcp and not huge:
            kinds += ["forecast"]
            if n <= 5000:
                kinds += ["forecast_posterior"]
        if st.after_run_more:
            kinds += ["last_device_us"] * 3
        k = rng.choice(kinds)
        if k == "summary":
            return op(k, rng.choice((0.975, 0.5, 0.9, 1.0, 0.25 / n, 0.25 / n)))    # (the last: floor(interval N) = 0, the rank clamps)
        if k == "forecast":
            cap = rng.choice((0, 1 + int(2 * (spec.dim() + 2) * n * 8 / 1024)))   # two horizons per chunk
            return op(k, rng.choice((2, 5)) if not big else 2, rng.randrange(1 << 30) if rng.random() < 0.5 else None,
                      rng.choice((0.975, 0.9)), cap)
        if k == "forecast_posterior":
            return op(k, 3, rng.randrange(1 << 30))
        return op(k)

    while len(seq) < length:
        if not st.initialised or st.failed or st.resampler_pending:
            r = rng.random()
            if not st.initialised and not st.resampler_pending and r < 0.25:
                inner = rng.choice((op("step", 1.0, 1.0, 1), op("run_more", 2, 5), op("summary", 0.975)))
                emit(op("refused", "ESTATE", inner))
            elif r < 0.4:
                emit(rng.choice((op("reseed", rng.randrange(1 << 40)), op("set_params", rng.randrange(4)), an_option())))
            else:
                emit(a_restart())
            continue
        r = rng.random()
        if st.pending_adopt and r < 0.6:
            emit(op("adopt", rng.choice((0.0, 0.3125, 0.9990234375))))
        elif r < 0.30:
            emit(a_step())
        elif r < 0.36:
            emit(a_step("propagate"))
        elif r < 0.44:
            T = run_length()
            emit(op("run_more", min(T, 60) if n > 1000 else T, rng.randrange(1000)))
        elif r < 0.52:
            emit(a_restart())
        elif r < 0.57:
            emit(op("set_params", rng.randrange(4)))
        elif r < 0.61:
            emit(op("reseed", rng.randrange(1 << 40)))
        elif r < 0.72:
            emit(an_option())
        elif r < 0.75:
            emit(op("set_option", OPT_RESAMPLER, rng.choice((0, 1, 2))))
        elif r < 0.78 and not spec.lgcp:
            emit(op("fails", "ENONFINITE", op("step", st.t - 1.0, _y(spec, rng), 1)))
        elif r < 0.83:
            emit(rng.choice((op("refused", "EINVAL_ARG", op("set_option", OPT_RESAMPLER, 7)),
                             op("refused", "EINVAL_ARG", op("run", 0, 0, 0)),
                             op("refused", "EINVAL_ARG", op("run_more", 0, 0)),
                             op("refused", "EINVAL_DESC", op("set_params_other")))))
        else:
            emit(a_read())
    # a sequence ends on a running filter that has just stepped: the last switch is followed by a step, the last state is compared
    if st.resampler_pending or not st.usable():
        emit(op("init", 0.0))
    emit(op("step", st.t + (0.25 if spec.lgcp else 1.0), _y(spec, rng), 1))
    return seq


# ---- deterministic completion of the pair table
def pair_allowed(spec: Spec, a: str, b: str) -> bool:
    """Whether the documented state machine lets state-changing kind b follow kind a DIRECTLY (in some state)."""
    if spec.lgcp and "interpolate" in (a, b):
        return False
    if a == "opt2" and b in ("step", "propagate", "adopt", "run_more"):
        return False                     # (a changed resampler is followed by a new cloud: the oracle takes it as a constructor flag)
    if a == "interpolate" and b in ("step", "propagate", "adopt", "run_more"):
        return False                     # the handle must be re-initialised first
    if b == "adopt" and a in ("init", "init_from", "step", "adopt", "run", "run_more"):
        return False                     # adopt follows a weighted propagate (options, parameters and the key may change in between)
    return True


def pair_snippet(spec: Spec, a: str, b: str, salt: int) -> List[Op]:
    """A short legal run that starts from ANY state, brings the handle where a then b may follow each other directly, and ends with
    a weighted step and a look at the cloud (so that what the pair left behind shows)."""
    dt = 0.25 if spec.lgcp else 1.0
    y = 1.0 if spec.data != "gaussian" else 0.5

    def make(kind: str, t: float, alt: int) -> Tuple[List[Op], float]:
        if kind == "init":
            return [op("init", 1.0)], 1.0
        if kind == "init_from":
            return [op("init_from", 0.5, 0.25)], 0.5
        if kind in ("step", "propagate"):
            return [op(kind, t + dt, y + 1.0, 1)], t + dt
        if kind == "adopt":
            return [op("adopt", 0.3125)], t
        if kind in ("run", "run_more", "interpolate"):
            T, ds = 3 + alt, 11 + salt
            tt = series(spec, T, ds, float(ds % 3) if kind != "run_more" else t, kind == "run_more")[0]
            o = op("run", T, ds, alt) if kind == "run" else (op("run_more", T, ds) if kind == "run_more" else op("interpolate", T, ds, 0.975))
            return [o], float(tt[-1])
        if kind == "set_params":
            return [op("set_params", 1 + (salt + alt) % 3)], t
        if kind == "reseed":
            return [op("reseed", 1000 + 7 * salt + alt)], t
        k = int(kind[3:])
        vals = OPTION_VALUES[k]
        return [op("set_option", k, vals[(salt + alt + 1) % len(vals)])], t

    out: List[Op] = [op("set_option", OPT_RESAMPLER, 0), op("init", 0.0), op("step", dt, y, 1)]
    t = dt
    if b == "adopt" and a != "propagate" or a == "adopt":
        out.append(op("propagate", t + dt, y, 1)); t += dt
    for kind, alt in ((a, 0), (b, 1)):
        ops, t = make(kind, t, alt)
        out += ops
    st = check_legal(spec, out)
    if st.resampler_pending or not st.usable():
        out.append(op("init", t)); st = check_legal(spec, out)
    out += [op("step", st.t + dt, y + 2.0, 1), op("particles")]
    return out


# The committed list: (seed, model, N, length).  Sizes where the geometry changes; CSSM_GRP_MIN_UNITS = 2 is set for every one of
# them by the GPU test (so group sums run from two units on).  The last two run at the library's own thresholds and are `slow`.
SEQUENCES: List[Tuple[int, str, int, int]] = [
    (1, "c1", 1, 40), (2, "c1", 2, 40), (3, "c1", 63, 45), (4, "c1", 1000, 45), (5, "c1", 1025, 40), (6, "c1", 5000, 40),
    (7, "c1", 70 * 1024 + 3, 22),
    (11, "c2", 1, 40), (12, "c2", 63, 45), (13, "c2", 1000, 50), (14, "c2", 1025, 40), (15, "c2", 5000, 40), (16, "c2", 70 * 1024 + 3, 22),
    (21, "c3", 2, 40), (22, "c3", 1000, 40), (23, "c3", 1025, 35), (24, "c3", 5000, 30), (25, "c3", 70 * 1024 + 3, 14),
    (31, "linear", 63, 45), (32, "linear", 1025, 40), (33, "linear", 5000, 40),
    (41, "studentt", 1000, 45), (42, "negbin", 1025, 40), (43, "negbin", 5000, 30),
    (51, "c4p1", 63, 40), (52, "c4p1", 1025, 40), (53, "c4p1", 5000, 30), (54, "c4p2", 1000, 25),
    (61, "rtc", 1000, 45), (62, "rtc", 5000, 40), (63, "rtc", 70 * 1024 + 3, 16),
]
SLOW_SEQUENCES: List[Tuple[int, str, int, int]] = [(71, "c1", (1 << 20) + 77, 15), (72, "c2", 1 << 20, 15)]
COMPLETION = ("c2", 1000)        # model and size of the sequences that hold the pairs the seeded draws left out
COMPLETION_CHUNK = 12            # pair snippets per completion sequence
SMOOTH_TWIN_PER_STEP = 4         # backward weights of the smoother twin (one Gaussian density each) that cost what one particle-step costs
FORECAST_ROW_COST = 2            # particle-steps per particle of one forecast row's expectation (init_from of a new oracle, one transition)
BUDGET = 6e7                     # particle-steps of fresh replay of the non-slow sequences together (about a minute of oracle time)


def pair_table(seqs: Sequence[Sequence[Op]]) -> Dict[Tuple[str, str], int]:
    tab: Dict[Tuple[str, str], int] = {}
    for seq in seqs:
        for x, y in zip(seq, seq[1:]):
            a, b = state_kind(x), state_kind(y)
            if a is not None and b is not None:
                tab[(a, b)] = tab.get((a, b), 0) + 1
    return tab


_committed = None


def committed_sequences():
    """[(id, spec name, n, ops, slow)]: the seeded sequences, then the completion sequences -- every allowed pair of state-changing
    kinds the seeded ones left out, as snippets in a fixed order."""
    global _committed
    if _committed is None:
        out = [(f"s{seed}-{name}-{n}", name, n, sequence(seed, name, n, length), False) for seed, name, n, length in SEQUENCES]
        out += [(f"s{seed}-{name}-{n}", name, n, sequence(seed, name, n, length), True) for seed, name, n, length in SLOW_SEQUENCES]
        spec = SPECS[COMPLETION[0]]
        tab = pair_table([s[3] for s in out])
        kinds = [k for k in STATE_KINDS]
        missing = [(a, b) for a in kinds for b in kinds if pair_allowed(spec, a, b) and (a, b) not in tab]
        for c in range(0, len(missing), COMPLETION_CHUNK):
            ops: List[Op] = []
            for i, (a, b) in enumerate(missing[c:c + COMPLETION_CHUNK]):
                ops += pair_snippet(spec, a, b, c + i)
            out.append((f"pairs{c // COMPLETION_CHUNK}-{COMPLETION[0]}-{COMPLETION[1]}", COMPLETION[0], COMPLETION[1], ops, False))
        _committed = out
    return _committed


# --------------------------------------------------------------------------------------------- the V2 generator
V2_INTERVALS = (0.975, 0.9, 1.0)


def sequence_v2(seed: int, spec_name: str, n: int, length: int, max_T: int = 0) -> List[Op]:
    """`length` ops of BOTH vocabularies on one handle, the V2 kinds about half of them: a function of its arguments alone (a
    random.Random of its own: sequence() is not touched).  max_T > 0 bounds every series length."""
    spec = SPECS[spec_name]
    rng = random.Random(f"call-sequences-v2/{seed}/{spec_name}/{n}/{length}/{max_T}")
    st = HostState(spec)
    small = n <= 5000                    # smooth and pmmh stay at n <= 5000 (their expectation is the slowest)
    big = n > 20000
    seq: List[Op] = []
    rows_calls = smooths = 0
    last_smooth_T = 0
    after_long = [False]                 # a call of more than 1024 records is followed by a new cloud (its replay at every checkpoint is dear)

    def emit(o: Op):
        st.apply(o)
        seq.append(o)

    def an_interval():
        return rng.choice(V2_INTERVALS + (0.975, 0.25 / n))        # (the last: floor(interval N) = 0, the rank clamps)

    def a_T(long_ok=True):
        nonlocal rows_calls
        rows_calls += 1
        if max_T:
            return rng.choice(range(1, max_T + 1))
        if big:
            return rng.choice((1, 2, 3, 4))
        if long_ok and 63 <= n <= 1000 and spec.precision != 2 and rows_calls == 3:
            after_long[0] = True
            return 1030 + rng.randrange(20)                         # behind a shorter rows call: the record and row buffers regrow
        return rng.choice((1, 2, 3, 5, 7, 12))

    def an_outlier(T):
        return rng.randrange(T) if (not spec.lgcp and rng.random() < 0.3) else None

    def next_t():
        return st.t + rng.choice(_DTS_LGCP if spec.lgcp else _DTS)

    def step_args():
        r = rng.random()
        if spec.lgcp:
            return next_t(), 1.0, 1
        if r < 0.15:
            return next_t(), 0.0, 0
        if r < 0.25:
            return st.t, _y(spec, rng), 1
        if r < 0.37:
            return next_t(), spec.outlier, 1
        return next_t(), _y(spec, rng), 1

    def rows_batch(kind):
        T = a_T()
        if T > 1024 and n > 513:
            kind = kind.replace("forecasts", "intervals")           # (a forecast row's expectation is a new oracle per record: kept to the smaller clouds)
        if kind.startswith("run_intervals"):
            return op(kind, T, rng.randrange(1000), an_interval(), an_outlier(T))
        return op(kind, T, rng.randrange(1000), int(rng.random() < 0.5), an_interval(), an_outlier(T))

    def a_smooth():
        nonlocal smooths, last_smooth_T
        smooths += 1
        T = rng.choice((2, 3, 5)) if last_smooth_T >= 9 else rng.choice((3, 9, 12, 12))    # a shorter one behind a longer one
        if max_T:
            T = min(T, max_T)
        last_smooth_T = T
        return op("smooth", T, rng.randrange(1000), rng.choice((1, 7, 63, 64)), an_interval())

    def a_pmmh():
        return op("pmmh", min(rng.choice((2, 4, 6)), max_T or 6), rng.randrange(1000), rng.choice((1, 2, 4)), rng.choice((0.01, 0.0025)),
                  rng.randrange(1 << 30))

    def a_restart():
        kinds = ["run_intervals"] * 3 + ["init", "run"]
        if not spec.lgcp:
            kinds += ["run_forecasts"] * 3
            if small:
                kinds += ["smooth"] * 2
        if small and not st.cloud_unknown:
            kinds += ["pmmh"] * 2
        k = rng.choice(kinds)
        if k == "init":
            return op("init", float(rng.choice((0.0, 1.0, 2.5))))
        if k == "run":
            return op("run", min(a_T(False), 25), rng.randrange(1000), 0)
        if k == "smooth":
            return a_smooth()
        if k == "pmmh":
            return a_pmmh()
        return rows_batch(k)

    def a_refusal():
        running, lg = st.usable(), spec.lgcp
        pool = [op("refused", "EINVAL_ARG", op("run_intervals", 0, 0, 0.975, None)),
                op("refused", "EINVAL_ARG", op("run_intervals", 3, 1, rng.choice((0.0, 1.5)), None)),
                op("refused", "EINVAL_ARG", op("run_forecasts", 0, 0, 0, 0.975, None)),
                op("refused", "EINVAL_ARG", op("run_forecasts", 3, 1, 0, rng.choice((0.0, 1.5)), None)),
                op("refused", "EINVAL_ARG", op("smooth", 3, 1, 0, 0.975)),
                op("refused", "EINVAL_ARG", op("smooth", 3, 1, 8, rng.choice((0.0, 1.5)))),
                op("refused", "EINVAL_ARG", op("smooth_pairing", 3, 1, 8, 0.975))]
        if lg:
            pool += [op("refused", "EINVAL_ARG", op("smooth", 3, 1, 8, 0.975))] * 6 + [op("refused", "EINVAL_ARG", op("run_forecasts", 3, 1, 0, 0.975, None))] * 3
        if running:
            pool += [op("refused", "EINVAL_ARG", op("run_intervals_more", 0, 0, 0.975, None)),
                     op("refused", "EINVAL_ARG", op("run_intervals_more", 2, 1, rng.choice((0.0, 1.5)), None)),
                     op("refused", "EINVAL_ARG", op("step_intervals", st.t + 1.0, 1.0, 1, rng.choice((0.0, 1.5)))),
                     op("refused", "EINVAL_ARG", op("run_forecasts_more", 0, 0, 0, 0.975, None)),
                     op("refused", "EINVAL_ARG", op("run_forecasts_more", 2, 1, 0, rng.choice((0.0, 1.5)), None)),
                     op("refused", "EINVAL_ARG", op("step_forecast", st.t + 1.0, 1.0, 1, None, rng.choice((0.0, 1.5))))]
            if lg:
                pool += [op("refused", "EINVAL_ARG", op("run_forecasts_more", 2, 1, 0, 0.975, None)),
                         op("refused", "EINVAL_ARG", op("step_forecast", st.t + 1.0, 1.0, 1, None, 0.975))] * 3
        return rng.choice(pool)

    def a_read():
        kinds = ["summary", "particles", "ancestors", "observation_index", "forecast_key", "proposed"]
        if st.weighted:
            kinds += ["weights", "logw"]
        k = rng.choice(kinds)
        return op(k, an_interval()) if k == "summary" else op(k)

    while len(seq) < length:
        if st.cloud_unknown and (st.params_unknown or st.seed_unknown):
            r = rng.random()
            if r < 0.2:
                emit(a_refusal())
            elif r < 0.35:
                emit(op("set_option", *rng.choice(((3, 0), (3, 1), (6, 1), (6, 0), (10, 2), (10, 1), (7, 0), (7, 1)))))
            elif st.params_unknown and (r < 0.7 or not st.seed_unknown):
                emit(op("set_params", rng.randrange(4)))
            else:
                emit(op("reseed", rng.randrange(1 << 40)))
            continue
        if not st.usable() or st.resampler_pending or st.cloud_unknown:
            r = rng.random()
            if not st.initialised and not st.resampler_pending and r < 0.45:
                emit(op("refused", "ESTATE", rng.choice((op("run_intervals_more", 2, 5, 0.975, None), op("step_intervals", 1.0, 1.0, 1, 0.975),
                                                          op("run_forecasts_more", 2, 5, 0, 0.975, None), op("step_forecast", 1.0, 1.0, 1, None, 0.975)))))
            elif r < 0.4:
                emit(rng.choice((op("reseed", rng.randrange(1 << 40)), op("set_params", rng.randrange(4)),
                                 a_refusal() if not st.resampler_pending else op("set_option", 8, rng.choice((0, 1, 2))))))
            else:
                emit(a_restart())
            continue
        r = rng.random()
        if after_long[0]:
            after_long[0] = False
            emit(op("particles"))
            emit(a_restart())
        elif st.pending_adopt and r < 0.6:
            emit(op("adopt", rng.choice((0.0, 0.3125, 0.9990234375))))
        elif r < 0.10:
            emit(op("step_intervals", *step_args(), an_interval()))
        elif r < 0.20:
            emit(op("step_forecast", *step_args(), rng.randrange(1 << 30) if rng.random() < 0.5 else None, an_interval()) if not spec.lgcp else a_refusal())
        elif r < 0.29:
            emit(rows_batch("run_intervals_more"))
        elif r < 0.38:
            emit(rows_batch("run_forecasts_more") if not spec.lgcp else a_refusal())
        elif r < 0.50:
            emit(a_restart())
        elif r < 0.54:
            emit(op("step", *step_args()))
        elif r < 0.59:
            t, y, has = step_args()
            emit(op("propagate", t, y if y != spec.outlier else _y(spec, rng), has))
        elif r < 0.62:
            emit(op("run_more", min(a_T(False), 12), rng.randrange(1000)))
        elif r < 0.66:
            emit(op("set_params", rng.randrange(4)))
        elif r < 0.70:
            emit(op("reseed", rng.randrange(1 << 40)))
        elif r < 0.78:
            k = rng.choice([q for q in OPTION_VALUES if q != OPT_RESAMPLER])
            emit(op("set_option", k, rng.choice([v for v in OPTION_VALUES[k] if v != st.opts[k]])))
        elif r < 0.80:
            emit(op("set_option", OPT_RESAMPLER, rng.choice((0, 1, 2))))
        elif r < 0.84 and not spec.lgcp:
            emit(op("fails", "ENONFINITE", rng.choice((op("step_intervals", st.t - 1.0, _y(spec, rng), 1, 0.975),
                                                       op("step_forecast", st.t - 1.0, _y(spec, rng), 1, None, 0.975)))))
        elif r < 0.95:
            emit(a_refusal())
        else:
            emit(a_read())
    # as in sequence(): the end is a running filter that has just taken a weighted step of a V2 kind, and the last state is compared
    while st.cloud_unknown and (st.params_unknown or st.seed_unknown):
        emit(op("set_params", 1) if st.params_unknown else op("reseed", 4242))
    if st.resampler_pending or not st.usable() or st.cloud_unknown:
        emit(op("init", 0.0))
    emit(op("step_intervals", st.t + (0.25 if spec.lgcp else 1.0), _y(spec, rng), 1, 0.975))
    return seq


def pair_allowed_v2(spec: Spec, a: str, b: str) -> bool:
    """pair_allowed over STATE_KINDS_V2: whether kind b may follow kind a DIRECTLY in some state."""
    new_a, new_b = a in NEW_KINDS, b in NEW_KINDS
    if not new_a and not new_b:
        return pair_allowed(spec, a, b)
    lgcp_refused = FORECAST_KINDS + ("smooth", "interpolate")
    if spec.lgcp and (a in lgcp_refused or b in lgcp_refused):
        return False
    needs_running = ("step", "propagate", "adopt", "run_more") + CONTINUING
    if a in ("opt2", "interpolate", "smooth") and b in needs_running:
        return False                     # a new cloud comes first
    if a == "pmmh":
        return b in ("set_params", "reseed") or b.startswith("opt")     # parameters and key are unknown: both are set, then a new cloud
    if b == "adopt":
        return a == "propagate" or a in ("set_params", "reseed") or a.startswith("opt")
    return True


def pair_snippet_v2(spec: Spec, a: str, b: str, salt: int) -> List[Op]:
    """pair_snippet over STATE_KINDS_V2: from a clean running state to a then b directly, then a weighted step and a look at the cloud."""
    dt = 0.25 if spec.lgcp else 1.0
    y = 1.0 if spec.data != "gaussian" else 0.5
    iv = V2_INTERVALS[salt % 3]

    def make(kind: str, t: float, alt: int) -> Tuple[Op, float]:
        T, ds = 3 + alt, 11 + salt
        if kind == "init":
            return op("init", 1.0), 1.0
        if kind == "init_from":
            return op("init_from", 0.5, 0.25), 0.5
        if kind in ("step", "propagate"):
            return op(kind, t + dt, y + 1.0, 1), t + dt
        if kind == "step_intervals":
            return op(kind, t + dt, y + 1.0, 1, iv), t + dt
        if kind == "step_forecast":
            return op(kind, t + dt, y + 1.0, 1, None if (salt + alt) % 2 else 977 + salt, iv), t + dt
        if kind == "adopt":
            return op("adopt", 0.3125), t
        if kind == "set_params":
            return op("set_params", 1 + (salt + alt) % 3), t
        if kind == "reseed":
            return op("reseed", 1000 + 7 * salt + alt), t
        if kind.startswith("opt"):
            k = int(kind[3:])
            vals = OPTION_VALUES[k]
            return op("set_option", k, vals[(salt + alt + 1) % len(vals)]), t
        o = {"run": op("run", T, ds, alt), "run_more": op("run_more", T, ds), "interpolate": op("interpolate", T, ds, 0.975),
             "run_intervals": op(kind, T, ds, iv, None), "run_intervals_more": op(kind, T, ds, iv, (salt % T) if salt % 4 == 0 and not spec.lgcp else None),
             "run_forecasts": op(kind, T, ds, (salt + alt) % 2, iv, None), "run_forecasts_more": op(kind, T, ds, (salt + alt) % 2, iv, None),
             "smooth": op(kind, T, ds, 16 + salt % 5, iv), "pmmh": op(kind, T, ds, 2, 0.01, 500 + salt)}[kind]
        return o, float(data_of(spec, o, t)[0][-1])

    out: List[Op] = [op("set_option", OPT_RESAMPLER, 0), op("init", 0.0), op("step", dt, y, 1)]
    t = dt
    if b == "adopt" and a != "propagate" or a == "adopt":
        out.append(op("propagate", t + dt, y, 1)); t += dt
    for kind, alt in ((a, 0), (b, 1)):
        o, t = make(kind, t, alt)
        out.append(o)
    st = check_legal(spec, out)
    if st.cloud_unknown:
        out += ([op("set_params", 0)] if st.params_unknown else []) + ([op("reseed", 20260101 + salt)] if st.seed_unknown else [])
    if st.resampler_pending or not st.usable() or st.cloud_unknown:
        out.append(op("init", t))
    st = check_legal(spec, out)
    out += [op("step_intervals", st.t + dt, y + 2.0, 1, 0.975) if salt % 2 else op("step", st.t + dt, y + 2.0, 1), op("particles")]
    return out


# (seed, model, N, length, max_T).  1, 2, 63: the smallest clouds; 512 / 513: the block edge of the pair kernel k_forecast_row; 1000: the
# mid size; 4097: above CSSM_IV_CAP; 5000: the largest size of smooth and pmmh; 70 * 1024 + 3: group sums; (c2, 131073): the second turn of
# k_fc_finish's block-strided loops; (c1, 300001), slow: the summary's grid-stride loops.
SEQUENCES_V2: List[Tuple[int, str, int, int, int]] = [
    (101, "c1", 1, 40, 0), (102, "c1", 63, 40, 0), (103, "c1", 513, 40, 0), (104, "c1", 1000, 45, 0), (105, "c1", 5000, 35, 0),
    (111, "c2", 2, 40, 0), (112, "c2", 512, 40, 0), (113, "c2", 1000, 45, 0), (114, "c2", 4097, 35, 0), (115, "c2", 70 * 1024 + 3, 13, 0),
    (121, "c3", 63, 40, 0), (122, "c3", 513, 35, 0), (123, "c3", 5000, 30, 0),
    (131, "linear", 2, 40, 0), (132, "linear", 1000, 45, 0), (133, "linear", 4097, 35, 0),
    (141, "studentt", 512, 40, 0), (142, "negbin", 1000, 40, 0), (143, "negbin", 5000, 30, 0),
    (151, "c4p1", 63, 35, 0), (152, "c4p1", 1000, 35, 0), (153, "c4p1", 4097, 25, 0), (154, "c4p1", 513, 40, 0),
    (161, "rtc", 513, 40, 0), (162, "rtc", 1000, 40, 0), (163, "rtc", 5000, 30, 0),
    (171, "c2", 131073, 10, 3),
]
SLOW_SEQUENCES_V2: List[Tuple[int, str, int, int, int]] = [(181, "c1", 300001, 11, 3)]

_committed_v2 = None


def pair_table_v2(seqs: Sequence[Sequence[Op]]) -> Dict[Tuple[str, str], int]:
    """pair_table restricted to the pairs with a V2 kind in them."""
    return {p: c for p, c in pair_table(seqs).items() if p[0] in NEW_KINDS or p[1] in NEW_KINDS}


def option_sweep_v2() -> List[Op]:
    """Every documented value of every option, followed by one of the V2 weighted kinds in turn before that option changes again."""
    out: List[Op] = [op("init", 0.0), op("step", 1.0, 2.0, 1)]
    i = 0
    for k, vals in OPTION_VALUES.items():
        for v in vals + (OPTION_DEFAULTS[k],):
            out.append(op("set_option", k, v))
            t = check_legal(SPECS[COMPLETION[0]], out).t
            new_cloud = (op("run_intervals", 3, 40 + i, 0.9, 1), op("run_forecasts", 3, 40 + i, 0, 0.975, None), op("smooth", 4, 40 + i, 9, 0.9),
                         op("run_forecasts", 2, 40 + i, 1, 1.0, 0))
            going_on = (op("step_intervals", t + 1.0, 3.0, 1, 0.975), op("run_forecasts_more", 3, 40 + i, 0, 0.9, 2), op("step_forecast", t + 0.5, 1.0, 1, None, 0.9),
                        op("run_intervals_more", 3, 40 + i, 1.0, 0))
            if k == OPT_RESAMPLER:
                out.append(new_cloud[i % 4])
                if new_cloud[i % 4].kind == "smooth":
                    out.append(op("init", 0.0))
            else:
                out.append(going_on[i % 4])
            i += 1
    return out + [op("step_intervals", check_legal(SPECS[COMPLETION[0]], out).t + 1.0, 2.0, 1, 0.975), op("particles")]


def committed_sequences_v2():
    """[(id, spec name, n, ops, slow)] of the second vocabulary: the seeded sequences, the option sweep, then the completion sequences
    -- every pair pair_allowed_v2 allows with a V2 kind in it that the seeded ones left out, as snippets in a fixed order."""
    global _committed_v2
    if _committed_v2 is None:
        out = [(f"v{seed}-{name}-{n}", name, n, sequence_v2(seed, name, n, length, mt), False) for seed, name, n, length, mt in SEQUENCES_V2]
        out += [(f"v{seed}-{name}-{n}", name, n, sequence_v2(seed, name, n, length, mt), True) for seed, name, n, length, mt in SLOW_SEQUENCES_V2]
        out.append((f"voptions-{COMPLETION[0]}-{COMPLETION[1]}", COMPLETION[0], COMPLETION[1], option_sweep_v2(), False))
        spec = SPECS[COMPLETION[0]]
        tab = pair_table([s[3] for s in out])
        missing = [(a, b) for a in STATE_KINDS_V2 for b in STATE_KINDS_V2
                   if (a in NEW_KINDS or b in NEW_KINDS) and pair_allowed_v2(spec, a, b) and (a, b) not in tab]
        for c in range(0, len(missing), COMPLETION_CHUNK):
            ops: List[Op] = []
            for i, (a, b) in enumerate(missing[c:c + COMPLETION_CHUNK]):
                ops += pair_snippet_v2(spec, a, b, c + i)
            out.append((f"vpairs{c // COMPLETION_CHUNK}-{COMPLETION[0]}-{COMPLETION[1]}", COMPLETION[0], COMPLETION[1], ops, False))
        _committed_v2 = out
    return _committed_v2


# --------------------------------------------------------------------------------------------- the expectation
def adopt_inputs(proposed: np.ndarray, logw: np.ndarray, u: float, ll_prev: float):
    """What a host resampler hands cssm_pf_adopt (model/ParticleFilter.scala:124-130): systematic ancestors of w1 = exp(w - max)
    (oracle.resample_systematic), the resampled cloud, the new ll and ESS."""
    mx = float(np.max(logw))
    w1 = oracle.c_exp(logw - mx)
    anc = oracle.resample_systematic(w1, u)
    q = w1 / np.sum(w1)
    return np.ascontiguousarray(proposed[:, anc]), ll_prev + mx + math.log(float(np.mean(w1))), int(math.floor(1.0 / float(np.sum(q * q))))


class Failed(Exception):
    """A call returned a status (subject or reference side)."""

    def __init__(self, code):
        super().__init__(f"status {code}")
        self.code = code


def _oracle_call(f, *a):
    try:
        return f(*a)
    except oracle.OracleError as e:
        raise Failed(ENONFINITE if e.code == oracle.ENONFINITE else e.code) from None


def _rows6(rows):
    return tuple(np.array([r[q] for r in rows]) for q in range(6))


def summary_row(o: oracle.OraclePf, interval: float):
    """The oracle's summary with its two means formed exactly (math.fsum over its cloud; eta_of_mean = its eta_of of that mean).  The
    oracle adds the N values one after the other: behind a record whose level was ruled out the cloud is N copies of a few particles,
    every addition rounds the same way, and the sum is off by up to N eps / 2 relative -- 7e-12 at N = 131073, measured 2.6e-12 --
    which is more than the 1e-12 the means are held to.  The order statistics are the oracle's own."""
    _, lo, hi, _, el, eu = o.summary(interval)
    m = np.array([math.fsum(row) for row in o.particles()]) / o.n
    return m, lo, hi, o.eta_of(m), el, eu


def _stepped(o: oracle.OraclePf, t, y, has, st: HostState, new_cloud: bool, interval=None, hook=None):
    """The route the rows calls replaced, on the oracle: [init; summary;] (step; summary)*.  `hook(s, cloud, clock, observation index,
    t_s, y_s, has_s)` sees the cloud BEFORE record s is stepped (the source of that record's forecast row).  (ll_t, ess_t, rows)."""
    rows = []
    clock, obs = st.t, st.obs
    if new_cloud:
        clock, obs = float(np.min(t)), 0
        o.init(clock)
        if interval is not None:
            rows.append(summary_row(o, interval))
    ll_t, ess_t = np.zeros(len(t)), np.zeros(len(t), dtype=np.int32)
    for s in range(len(t)):
        if hook is not None:
            hook(s, o.particles(), clock, obs + s, float(t[s]), float(y[s]), bool(has[s]))
        ll_t[s], ess_t[s] = _oracle_call(o.step, float(t[s]), float(y[s]), bool(has[s]))
        clock = float(t[s])
        if interval is not None:
            rows.append(summary_row(o, interval))
    return ll_t, ess_t, rows


def smooth_expected(o: oracle.OraclePf, model: Model, n: int, seed: int, t, y, has, M: int, interval: float):
    """What cssm_pf_smooth returns, from the oracle `o` (of `model`, n particles, key `seed`): ll of its interpolate (the header: the
    forward pass is that code), the backward simulation of the sequential twin on its history (the route of test_gpu_smooth.twin_of),
    the oracle's summary of the states the trajectories pass through.  (ll, mean, lower, upper, eta_of_mean, eta_lower, eta_upper, traj)"""
    from test_fleet_smooth_host import kinds_of, pack_records, twin_traj
    from test_smooth_host import twin_rows
    ll = _oracle_call(o.interpolate, t, y, has, interval)[0]
    o.init(float(np.min(t)))
    X, Anc, ll_h = [o.particles()], [o.ancestors()], 0.0
    for s in range(len(t)):
        ll_h, _ = _oracle_call(o.step, float(t[s]), float(y[s]), bool(has[s]))
        X.append(o.proposed()); Anc.append(o.ancestors())
    if ll_h != ll:
        raise StaleOracle(f"the oracle's interpolate ll {ll!r} is not its stepped history's {ll_h!r}")
    X = np.array(X)
    traj = twin_traj(X, np.array(Anc), pack_records(model, n, seed, t, y, has), kinds_of(model), seed, M)
    return (ll,) + twin_rows(model, X, traj, t, interval) + (traj,)


def apply_to_oracle(o: oracle.OraclePf, spec: Spec, x: Op, st: HostState, ll_prev: float, rows: bool = False, hook=None):
    """One state-changing op on an initialised oracle; returns what the call returns.  `st` is the state BEFORE the op.  `rows`: form
    the summary rows of the V2 interval kinds too, `hook`: see _stepped (a replay at a checkpoint wants neither)."""
    k = x.kind
    if k in ROW_KINDS:
        if k in STEP_ROWS:
            t, y, has = np.array([x[1]]), np.array([x[2]]), np.array([x[3]], dtype=np.uint8)
        else:
            t, y, has = data_of(spec, x, st.t)
        iv = interval_of(x) if (rows and k in INTERVAL_KINDS) else None
        ll_t, ess_t, r = _stepped(o, t, y, has, st, k in NEW_RESTARTS, iv, hook)
        if k in STEP_ROWS:
            return (float(ll_t[0]), int(ess_t[0])) + (tuple(r[0]) if r else ())
        return (float(ll_t[-1]), ll_t, ess_t) + (_rows6(r) if r else ())
    if k == "init":
        o.init(x[1]); return (0.0, o.n)
    if k == "init_from":
        o.init_from(x[1], np.full(o.d, x[2]) * (1.0 + np.arange(o.d)) / o.d); return (0.0, o.n)
    if k == "step":
        return _oracle_call(o.step, x[1], x[2], bool(x[3]))
    if k == "propagate":
        o.propagate_only(x[1], x[2], bool(x[3]))
        prop = o.proposed()
        o.set_particles(prop)            # "After cssm_pf_propagate without cssm_pf_adopt the proposed cloud is the current one."
        return None
    if k == "adopt":
        cloud, ll, ess = adopt_inputs(o.proposed(), o.logw(), x[1], ll_prev)
        o.adopt(cloud, ll, ess)
        return (cloud, ll, ess)
    if k == "run":
        t, y, has = series(spec, x[1], x[2], float(x[2] % 3), False)
        return _oracle_call(o.filter, t, y, has, bool(x[3]))
    if k == "run_more":
        t, y, has = series(spec, x[1], x[2], st.t, True)
        ll_t, ess_t = np.zeros(len(t)), np.zeros(len(t), dtype=np.int32)
        for s in range(len(t)):
            ll_t[s], ess_t[s] = _oracle_call(o.step, float(t[s]), float(y[s]), bool(has[s]))
        return (float(ll_t[-1]), ll_t, ess_t)
    if k == "interpolate":
        t, y, has = series(spec, x[1], x[2], float(x[2] % 3), False)
        return _oracle_call(o.interpolate, t, y, has, x[3])
    if k == "set_params":
        o.set_params(spec.model(x[1]).descriptor(spec.precision)); return None
    if k == "reseed":
        o.reseed(x[1]); return None
    raise AssertionError(f"not an oracle op: {x!r}")


class StaleOracle(AssertionError):
    pass


class Ref:
    """The expectation.  The live prefix = the state-changing ops since the last call that drew a new cloud, under the model, key
    and resampler of that moment; `o` is an OraclePf that has replayed exactly that prefix.  It is advanced op by op between
    checkpoints and thrown away at every checkpoint for a NEW object that replays the prefix from scratch (the two must agree:
    StaleOracle otherwise)."""

    def __init__(self, spec: Spec, n: int, seed: int):
        self.spec, self.n = spec, n
        self.st = HostState(spec)
        self.model_k, self.seed = 0, int(seed)
        self.base = None                 # (model_k, seed, resampler) of the prefix' first op
        self.prefix: List[Op] = []
        self.o: Optional[oracle.OraclePf] = None
        self.ll, self.ess = 0.0, n
        self.last_y: Optional[float] = None   # datum of the last weighted native step (None: LGCP, or none yet)
        self.wmode: Optional[str] = None      # "w", "log", or None where only the handle can tell
        self.particle_steps = 0
        self.hook = None                 # the runner's look at the cloud before every record of a forecast call (see _stepped)

    def _new(self) -> oracle.OraclePf:
        k, seed, rs = self.base
        return oracle.OraclePf(self.spec.model(k).descriptor(self.spec.precision), self.n, seed, RESAMPLER_FLAGS[rs])

    def _cost(self, x: Op, st: HostState, rows: bool = True) -> int:
        """Particle-steps of oracle work of one op (rows: with the expectation of a forecast call's rows, which a replay does not form)."""
        k = x.kind
        if k in ("step", "propagate"):
            return self.n * substeps(self.spec, x[1] - st.t)
        if k in ("run", "interpolate", "run_more"):
            t = series(self.spec, x[1], x[2], st.t if k == "run_more" else float(x[2] % 3), k == "run_more")[0]
            prev = np.concatenate(([st.t if k == "run_more" else t[0]], t[:-1]))
            return self.n * int(sum(substeps(self.spec, float(d)) for d in t - prev)) + (self.n if k != "run_more" else 0)
        if k in ("init", "init_from"):
            return self.n
        if k in STEP_ROWS:
            return self.n * (substeps(self.spec, x[1] - st.t) + (FORECAST_ROW_COST if k == "step_forecast" and rows else 0))
        if k in BATCH_ROWS or k in ("smooth", "pmmh"):
            cont = k in CONTINUING
            t = data_of(self.spec, x, st.t)[0]
            prev = np.concatenate(([st.t if cont else t[0]], t[:-1]))
            c = self.n * int(sum(substeps(self.spec, float(d)) for d in t - prev)) + (0 if cont else self.n)
            if k in FORECAST_KINDS and rows:
                c += FORECAST_ROW_COST * self.n * len(t)          # per row: a new oracle of the cloud, one transition
            if k == "smooth":
                c = 2 * c + x[3] * self.n * len(t) // SMOOTH_TWIN_PER_STEP   # interpolate, the stepped history, the twin: M trajectories x N parents
            if k == "pmmh":
                c *= x[3]
            return c
        return 0

    def _new_cloud_oracle(self) -> oracle.OraclePf:
        """A new oracle under the model, key and resampler of this moment."""
        return oracle.OraclePf(self.spec.model(self.model_k).descriptor(self.spec.precision), self.n, self.seed,
                               RESAMPLER_FLAGS[self.st.opts[OPT_RESAMPLER]])

    def _smooth(self, x: Op):
        t, y, has = data_of(self.spec, x, 0.0)
        return smooth_expected(self._new_cloud_oracle(), self.spec.model(self.model_k), self.n, self.seed, t, y, has, x[3], x[4])

    def _pmmh(self, x: Op):
        t, y, has = data_of(self.spec, x, 0.0)
        model = self.spec.model(self.model_k)
        return _oracle_call(self._new_cloud_oracle().pmmh, model.descriptor(self.spec.precision), theta_of(model), x[4], t, y, has, x[5], x[3])

    def apply(self, x: Op):
        """Advance by one legal op; returns the expected return value of a state-changing call (None otherwise)."""
        st = self.st
        k = x.kind
        exp = None
        if k == "fails":
            inner = x[2]
            try:
                apply_to_oracle(self.o, self.spec, inner, st, self.ll)
            except Failed as e:
                exp = e.code
            self.particle_steps += self._cost(inner, st)
            self.o = None
            self.prefix = []
        elif state_kind(x) is not None:
            if k == "set_option":
                pass
            elif k == "smooth":
                exp = self._smooth(x)
            elif k == "pmmh":
                exp = self._pmmh(x)
            elif k in ALL_RESTARTS:
                self.base = (self.model_k, self.seed, st.opts[OPT_RESAMPLER])
                self.prefix = [x]
                self.o = self._new()
                exp = apply_to_oracle(self.o, self.spec, x, st, 0.0, True, self.hook)
            else:
                if k == "set_params":
                    self.model_k = x[1]
                if k == "reseed":
                    self.seed = int(x[1])
                if self.o is not None and st.usable():
                    self.prefix.append(x)
                    exp = apply_to_oracle(self.o, self.spec, x, st, self.ll, True, self.hook)
            self.particle_steps += self._cost(x, st)
            self._track(x, exp)
        st.apply(x)
        if k in ("interpolate", "smooth", "pmmh"):
            self.o = None                # nothing of the cloud is defined until the handle is initialised again
            self.prefix = []
        return exp

    def _track(self, x: Op, exp):
        """ll / ESS of the filter, and whether the handle now keeps weights or log-weights (include/cssm_pf.h, cssm_pf_get_logw)."""
        k, sp, st = x.kind, self.spec, self.st
        if k in ("init", "init_from"):
            self.ll, self.ess, self.wmode = 0.0, self.n, "log"
        elif k == "step":
            self.ll, self.ess = exp
            if x[3] or sp.lgcp:
                self._mode_after_native(None if sp.lgcp else x[2])
        elif k in ("run", "run_more"):
            t, y, has = series(sp, x[1], x[2], st.t if k == "run_more" else float(x[2] % 3), k == "run_more")
            if k == "run":
                self.wmode = "log"
            self.ll = exp[0]
            self.ess = int(exp[2][-1])
            w = np.nonzero(has)[0]
            if len(w):
                self._mode_after_native(None if sp.lgcp else float(y[w[-1]]))
        elif k in STEP_ROWS:
            self.ll, self.ess = exp[0], exp[1]
            if x[3] or sp.lgcp:
                self._mode_after_native(None if sp.lgcp else x[2])
        elif k in BATCH_ROWS:
            t, y, has = data_of(sp, x, st.t)
            if k in NEW_RESTARTS:
                self.wmode = "log"
            self.ll = exp[0]
            self.ess = int(exp[2][-1])
            w = np.nonzero(has)[0]
            if len(w):
                self._mode_after_native(None if sp.lgcp else float(y[w[-1]]))
        elif k == "propagate":
            if x[3] or sp.lgcp:
                self.wmode = "log"       # the host resampler wants the log-weights themselves
        elif k == "adopt":
            self.ll, self.ess = exp[1], exp[2]

    def _mode_after_native(self, y):
        opts = self.st.opts
        if not opts[OPT_FUSED] or opts[OPT_RESAMPLER] == 2:
            self.wmode = "log"
        elif y is None:
            self.wmode = None            # LGCP: fused once a level is predicted, redone where the max rules it out
        else:
            level, _ = self.o.ref()
            self.wmode = "w" if level == self.o.ref_level(y) else "log"   # (another level than the observation's own: it was redone)

    def rebuild(self) -> None:
        """Checkpoint: a NEW oracle replays the live prefix; it must agree with the cached one, and replaces it."""
        if self.o is None:
            return
        fresh = self._new()
        st = HostState(self.spec)
        st.opts = dict(self.st.opts)
        ll = 0.0
        for x in self.prefix:
            r = apply_to_oracle(fresh, self.spec, x, st, ll)
            self.particle_steps += self._cost(x, st, rows=False)
            if x.kind in ("step",) + STEP_ROWS:
                ll = r[0]
            elif x.kind in ("run", "run_more") + BATCH_ROWS:
                ll = r[0]
            elif x.kind == "adopt":
                ll = r[1]
            elif x.kind in ("init", "init_from"):
                ll = 0.0
            st.apply(x)
        for name in ("particles", "ancestors", "logw"):
            a, b = getattr(fresh, name)(), getattr(self.o, name)()
            if name == "logw" and not self.st.weighted:
                continue
            if not np.array_equal(a, b, equal_nan=True):
                raise StaleOracle(f"the oracle carried through {len(self.prefix)} ops differs from a fresh replay in {name}() at "
                                  f"{int(np.sum(a != b))} entries: prefix {pasteable(self.prefix)}")
        if ll != self.ll:
            raise StaleOracle(f"ll of the carried oracle {self.ll!r} != fresh replay {ll!r}")
        self.o = fresh

    # -- expected views of the state
    def particles(self):
        return self.o.particles()

    def proposed(self):
        return self.o.particles() if self.st.last_cloud_kind == "adopt" else self.o.proposed()   # the adopted cloud replaced it in place

    def ancestors(self):
        if self.st.last_cloud_kind in ("propagate", "adopt"):
            return np.arange(self.n, dtype=np.uint32)      # no native resampling stands behind the current cloud
        return self.o.ancestors()

    def forecast_key(self):
        return int(oracle.lib().oracle_c_derive_key(self.seed, (1 << 63) | self.st.obs))


def replay_cost(spec_name: str, n: int, seq: Sequence[Op], checkpoints=True) -> int:
    """Particle-steps of oracle work the runner spends on `seq` (replays at checkpoints included), computed without running anything."""
    spec = SPECS[spec_name]
    r = Ref.__new__(Ref)
    r.spec, r.n = spec, n
    st = HostState(spec)
    total, prefix_cost = 0, 0
    pending_switch = False
    for i, x in enumerate(seq):
        inner = x[2] if x.kind == "fails" else x
        c = r._cost(inner, st) if (state_kind(inner) is not None and inner.kind != "set_option") else 0
        if x.kind in ("forecast", "forecast_posterior"):
            c = n * (x[1] if x.kind == "forecast" else 3 * 2)
        total += c
        if x.kind in ("smooth", "pmmh"):
            prefix_cost = 0
        elif x.kind in ALL_RESTARTS:
            prefix_cost = c - (FORECAST_ROW_COST * n * x[1] if x.kind == "run_forecasts" else 0)   # (a replay forms no rows)
        elif x.kind == "fails":
            prefix_cost = 0
        elif x.kind in FORECAST_KINDS:
            prefix_cost += c - FORECAST_ROW_COST * n * (1 if x.kind == "step_forecast" else x[1])
        elif state_kind(x) is not None:
            prefix_cost += c
        cp, pending_switch = _is_checkpoint(x, i == len(seq) - 1, pending_switch)
        st.apply(x)
        if cp and checkpoints and st.usable():
            total += prefix_cost
    return total


def _is_checkpoint(x: Op, last: bool, pending_switch: bool):
    """After every run, after the first step behind an option switch, and at the end."""
    k = x.kind
    if k == "set_option":
        return last, True
    if k in ("step", "run_more") + STEP_ROWS and pending_switch:
        return True, False
    if k == "run" or k in BATCH_ROWS:
        return True, False
    return last, pending_switch


# --------------------------------------------------------------------------------------------- subjects
class CarriedOracle:
    """ONE oracle.OraclePf carried through a whole sequence behind NativePf's method names (a new object only where the resampler
    changes: the oracle takes it as a constructor flag).  The subject of the CPU half: against it the runner checks that a reused
    oracle equals the fresh replay, i.e. that the expectation has no stale state of its own."""
    native = False

    def __init__(self, spec: Spec, n: int, seed: int):
        self.spec, self.n, self.seed, self.model, self.rs = spec, n, int(seed), spec.model(0), 0
        self.opts = dict(OPTION_DEFAULTS)
        self._make()
        self.d = self.o.d

    def _make(self):
        self.o = oracle.OraclePf(self.model.descriptor(self.spec.precision), self.n, self.seed, RESAMPLER_FLAGS[self.rs])
        self.init_ok, self.t, self.obs, self.ll, self.last = False, 0.0, 0, 0.0, None

    def _need_init(self):
        if not self.init_ok:
            raise Failed(ESTATE)

    def close(self):
        self.o = None

    def init(self, t0):
        self.o.init(t0); self.init_ok, self.t, self.obs, self.ll, self.last = True, t0, 0, 0.0, "init"

    def init_from(self, t0, state):
        self.o.init_from(t0, state); self.init_ok, self.t, self.obs, self.ll, self.last = True, t0, 0, 0.0, "init"

    def step(self, t, y, has):
        self._need_init()
        self.t, self.obs, self.last = t, self.obs + 1, "step"
        r = _oracle_call(self.o.step, t, y, bool(has))
        self.ll = r[0]
        return r

    def propagate(self, t, y, has):
        self._need_init()
        self.o.propagate_only(t, y, bool(has)); self.o.set_particles(self.o.proposed())
        self.t, self.obs, self.last = t, self.obs + 1, "propagate"

    def adopt(self, cloud, ll, ess):
        self.o.adopt(cloud, ll, ess); self.ll, self.last = ll, "adopt"

    def run(self, t, y, has, want_path=False):
        if len(t) < 1:
            raise Failed(EINVAL_ARG)
        r = _oracle_call(self.o.filter, t, y, has, want_path)
        self.init_ok, self.t, self.obs, self.ll, self.last = True, float(t[-1]), len(t), r[0], "run"
        return r

    def run_more(self, t, y, has):
        if len(t) < 1:
            raise Failed(EINVAL_ARG)
        self._need_init()
        ll_t, ess_t = np.zeros(len(t)), np.zeros(len(t), dtype=np.int32)
        for s in range(len(t)):
            ll_t[s], ess_t[s] = self.step(float(t[s]), float(y[s]), bool(has[s]))
        return float(ll_t[-1]), ll_t, ess_t

    def interpolate(self, t, y, has, interval):
        r = _oracle_call(self.o.interpolate, t, y, has, interval)
        self.init_ok = False
        return r

    def set_params(self, model, lgcp_precision=0):
        if sum(s.dimension for _, _, s in model.leaves) != self.d:
            raise Failed(EINVAL_DESC)     # (oracle_pf_set_params would have rebuilt its components before it noticed)
        self.model = model
        self.o.set_params(model.descriptor(lgcp_precision))

    def reseed(self, seed):
        self.seed = int(seed); self.o.reseed(self.seed)

    def set_option(self, k, v):
        if k == OPT_RESAMPLER:
            if v not in (0, 1, 2):
                raise Failed(EINVAL_ARG)
            if v != self.rs:
                self.rs = v
                self._make()
        self.opts[k] = v

    def summary(self, interval):
        self._need_init()
        return self.o.summary(interval)

    # -- the V2 calls: the route each of them replaced, on the carried object
    def _rows(self, t, y, has, interval, new_cloud, lgcp_refused=False):
        if not new_cloud:
            self._need_init()
        if (lgcp_refused and self.spec.lgcp) or len(t) < 1 or _bad_interval(interval):
            raise Failed(EINVAL_ARG)
        obs0 = 0 if new_cloud else self.obs
        try:
            ll_t, ess_t, rows = _stepped(self.o, t, y, has, self, new_cloud, None if lgcp_refused else interval)
        finally:
            self.init_ok, self.t, self.obs, self.last = True, float(t[-1]), obs0 + len(t), "run" if new_cloud else "step"
        self.ll = float(ll_t[-1])
        return (self.ll, ll_t, ess_t) + (_rows6(rows) if rows else ())

    def filter_intervals(self, t, y, has, interval):
        return self._rows(t, y, has, interval, True)

    def filter_intervals_more(self, t, y, has, interval):
        return self._rows(t, y, has, interval, False)

    def step_intervals(self, t, y, has, interval):
        self._need_init()
        if _bad_interval(interval):
            raise Failed(EINVAL_ARG)
        return self.step(t, y, has) + summary_row(self.o, interval)

    def default_forecast_keys(self, first, count):
        return np.array([int(oracle.lib().oracle_c_derive_key(self.seed, (1 << 63) | (first + s))) for s in range(count)], dtype=np.uint64)

    def _forecasts(self, t, y, has, keys, interval, new_cloud):
        if not new_cloud:
            self._need_init()
        used = self.default_forecast_keys(0 if new_cloud else self.obs, len(t)) if keys is None else np.asarray(keys, dtype=np.uint64)
        r = self._rows(t, y, has, interval, new_cloud, lgcp_refused=True)
        return dict(ll=r[0], ll_t=r[1], ess_t=r[2], keys=used)

    def filter_forecasts(self, t, y, has, keys, interval):
        return self._forecasts(t, y, has, keys, interval, True)

    def filter_forecasts_more(self, t, y, has, keys, interval):
        return self._forecasts(t, y, has, keys, interval, False)

    def step_forecast(self, t, y, has, key, interval):
        self._need_init()
        if self.spec.lgcp or _bad_interval(interval):
            raise Failed(EINVAL_ARG)
        used = self.forecast_key() if key is None else int(key)
        return self.step(t, y, has) + ({"key": used},)

    def smooth(self, t, y, has, n_traj, interval, want_trajectories=True, flags=0):
        if self.spec.lgcp or flags or not 1 <= n_traj <= SMOOTH_MAX_M or _bad_interval(interval) or len(t) < 1:
            raise Failed(EINVAL_ARG)
        try:
            return smooth_expected(self.o, self.model, self.n, self.seed, t, y, has, n_traj, interval)
        finally:
            self.init_ok = False

    def pmmh(self, model, delta, t, y, has, seed, iters):
        r = _oracle_call(self.o.pmmh, model.descriptor(self.spec.precision), theta_of(model), delta, t, y, has, seed, iters)
        self.init_ok, self.t, self.obs, self.last = True, float(t[-1]), len(t), "run"
        return r

    def particles(self):
        return self.o.particles()

    def proposed(self):
        return self.o.particles() if self.last == "adopt" else self.o.proposed()

    def ancestors(self):
        return np.arange(self.n, dtype=np.uint32) if self.last in ("propagate", "adopt") else self.o.ancestors()

    def weights(self):
        return None

    def logw(self):
        return self.o.logw()

    def observation_index(self):
        return self.obs

    def forecast_key(self):
        return int(oracle.lib().oracle_c_derive_key(self.seed, (1 << 63) | self.obs))


def _native_call(f, *a, **kw):
    from composablestatespacemodels_amd import CssmError
    try:
        return f(*a, **kw)
    except CssmError as e:
        if e.code == EHIP:
            raise                        # a HIP error ends the run: nothing is replayed, nothing goes on
        raise Failed(e.code) from None


def _native_smooth_raw(g, t, y, has, M, interval, flags):
    """cssm_pf_smooth itself, for the arguments NativePf.smooth refuses on the Python side (n_traj = 0, an interval outside (0, 1],
    CSSM_INTERP_REFERENCE_PAIRING): the status must be the library's."""
    import ctypes as C
    from composablestatespacemodels_amd import CssmError
    t, y = np.ascontiguousarray(t, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    has = np.ascontiguousarray(has, dtype=np.uint8)
    dp = C.POINTER(C.c_double)
    ll = C.c_double()
    rc = g.lib.cssm_pf_smooth(g._h, t.ctypes.data_as(dp), y.ctypes.data_as(dp), has.ctypes.data_as(C.POINTER(C.c_uint8)), len(t), int(M),
                              float(interval), int(flags), C.byref(ll), *([None] * 6), None)
    if rc:
        raise CssmError(rc, "cssm_pf_smooth")
    return (ll.value,)


def _native_pmmh(g, model, precision, delta, t, y, has, seed, iters):
    """cssm_pmmh_run on the handle of g (composablestatespacemodels_amd.pmmh.pmmh_native creates a handle of its own and closes it)."""
    import ctypes as C
    from composablestatespacemodels_amd import _abi
    t, y = np.ascontiguousarray(t, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    has = np.ascontiguousarray(has, dtype=np.uint8)
    theta0 = np.ascontiguousarray(theta_of(model))
    nt = theta0.size
    ll, th, acc, last = np.zeros(iters), np.zeros((iters, nt)), np.zeros(iters, dtype=np.int32), np.zeros((iters, g.d))
    dp = C.POINTER(C.c_double)
    desc = model.descriptor(precision)
    _abi.check(g.lib.cssm_pmmh_run(g._h, desc.ptr(), theta0.ctypes.data_as(dp), nt, float(delta), t.ctypes.data_as(dp), y.ctypes.data_as(dp),
                                   has.ctypes.data_as(C.POINTER(C.c_uint8)), len(t), int(seed), int(iters), ll.ctypes.data_as(dp),
                                   th.ctypes.data_as(dp), acc.ctypes.data_as(C.POINTER(C.c_int32)), last.ctypes.data_as(dp)))
    return ll, th, acc, last


# --------------------------------------------------------------------------------------------- the runner
class Divergence(AssertionError):
    pass


class _Mismatch(AssertionError):
    pass


def _eq(name, got, exp):
    got, exp = np.asarray(got), np.asarray(exp)
    if got.shape != exp.shape or not np.array_equal(got, exp, equal_nan=True):
        bad = int(np.sum(~((got == exp) | (np.isnan(got) & np.isnan(exp))))) if got.shape == exp.shape and got.dtype.kind == "f" else \
            (int(np.sum(got != exp)) if got.shape == exp.shape else -1)
        raise _Mismatch(f"{name} differs at {bad} of {exp.size} entries" + (f": got {got.tolist()!r}, expected {exp.tolist()!r}" if exp.size <= 4 else ""))


def _close(name, got, exp):
    try:
        np.testing.assert_allclose(got, exp, rtol=1e-12, atol=1e-13)      # (test_device_summaries_match_oracle's tolerance for means)
    except AssertionError as e:
        raise _Mismatch(f"{name}: {e}") from None


def _compare_summary(got, exp, what="summary"):
    gm, glo, ghi, gem, gel, geu = got
    om, olo, ohi, oem, oel, oeu = exp
    _eq(what + " lower", glo, olo); _eq(what + " upper", ghi, ohi)
    _eq(what + " eta lower", gel, oel); _eq(what + " eta upper", geu, oeu)
    _close(what + " mean", gm, om); _close(what + " eta of mean", gem, oem)


class Runner:
    def __init__(self, subject, spec_name: str, n: int, seed: int, twin=None, make_subject=None):
        self.g, self.spec, self.n, self.seed = subject, SPECS[spec_name], n, int(seed)
        self.native = getattr(subject, "native", True)
        self.ref = Ref(self.spec, n, seed)
        self.twin = twin
        self.make_subject = make_subject
        self.wall_us = None
        self.log: List[str] = []

    # -- one op on the subject, compared with the reference
    def _state_call(self, x: Op, st: HostState):
        """Run state-changing op x on the subject; returns what it returned."""
        g, sp, k = self.g, self.spec, x.kind
        call = _native_call if self.native else (lambda f, *a, **kw: f(*a, **kw))
        if k == "init":
            return call(g.init, x[1])
        if k == "init_from":
            return call(g.init_from, x[1], np.full(g.d, x[2]) * (1.0 + np.arange(g.d)) / g.d)
        if k == "step":
            return call(g.step, x[1], x[2], bool(x[3]))
        if k == "propagate":
            return call(g.propagate, x[1], x[2], bool(x[3]))
        if k == "run":
            t, y, has = series(sp, x[1], x[2], float(x[2] % 3), False)
            return call(g.run, t, y, has, bool(x[3]))
        if k == "run_more":
            t, y, has = series(sp, x[1], x[2], st.t, True)
            t0 = time.perf_counter()
            r = call(g.run_more, t, y, has)
            self.wall_us = (time.perf_counter() - t0) * 1e6
            return r
        if k == "interpolate":
            t, y, has = series(sp, x[1], x[2], float(x[2] % 3), False)
            return call(g.interpolate, t, y, has, x[3])
        if k == "set_params":
            return call(g.set_params, sp.model(x[1]), sp.precision)
        if k == "set_params_other":
            return call(g.set_params, sp.other_structure(), 0)
        if k == "reseed":
            return call(g.reseed, x[1])
        if k == "set_option":
            return call(g.set_option, x[1], x[2])
        if k == "summary":
            return call(g.summary, x[1])
        if k in ("run_intervals", "run_intervals_more"):
            t, y, has = data_of(sp, x, st.t)
            return call(g.filter_intervals if k == "run_intervals" else g.filter_intervals_more, t, y, has, x[3])
        if k == "step_intervals":
            return call(g.step_intervals, x[1], x[2], bool(x[3]), x[4])
        if k in ("run_forecasts", "run_forecasts_more"):
            t, y, has = data_of(sp, x, st.t)
            return call(g.filter_forecasts if k == "run_forecasts" else g.filter_forecasts_more, t, y, has,
                        row_keys(x[2], x[1]) if x[3] else None, x[4])
        if k == "step_forecast":
            return call(g.step_forecast, x[1], x[2], bool(x[3]), x[4], x[5])
        if k in ("smooth", "smooth_pairing"):
            t, y, has = data_of(sp, x, 0.0)
            flags = 1 if k == "smooth_pairing" else 0        # CSSM_INTERP_REFERENCE_PAIRING
            if self.native and (flags or not 1 <= x[3] <= SMOOTH_MAX_M or _bad_interval(x[4])):
                return call(_native_smooth_raw, g, t, y, has, x[3], x[4], flags)
            return call(g.smooth, t, y, has, x[3], x[4], True, **({} if self.native else {"flags": flags}))
        if k == "pmmh":
            t, y, has = data_of(sp, x, 0.0)
            model = sp.model(self.ref.model_k)
            if self.native:
                return call(_native_pmmh, g, model, sp.precision, x[4], t, y, has, x[5], x[3])
            return call(g.pmmh, model, x[4], t, y, has, x[5], x[3])
        raise AssertionError(f"not a state call: {x!r}")

    def _do(self, x: Op):
        ref, g, k = self.ref, self.g, x.kind
        st = ref.st
        call = _native_call if self.native else (lambda f, *a, **kw: f(*a, **kw))
        if k == "refused":
            want = CODES[x[1]]
            before = (st.initialised and not st.failed)
            try:
                self._state_call(x[2], st)
            except Failed as e:
                if e.code != want:
                    raise _Mismatch(f"refused with status {e.code}, the documented one is {want} ({x[1]})")
            else:
                raise _Mismatch(f"the call was accepted; documented: {x[1]}")
            ref.apply(x)
            if before:
                self._compare_cloud("after the refused call ")     # a refused call leaves the handle as it was
            return
        if k == "fails":
            want = ref.apply(x)
            try:
                self._state_call(x[2], HostState(self.spec))
            except Failed as e:
                if e.code != want or want != CODES[x[1]]:
                    raise _Mismatch(f"failed with status {e.code}; oracle {want}, documented {x[1]}")
            else:
                raise _Mismatch(f"the call succeeded; documented: {x[1]}")
            return
        if k == "adopt":
            exp = ref.apply(x)
            call(g.adopt, exp[0], exp[1], exp[2])
            return
        if k in FORECAST_KINDS:
            # the subject first: the reference then holds every row against the cloud it has BEFORE that record, as it steps
            pre = HostState.__new__(HostState); pre.__dict__.update(st.__dict__)
            got = self._state_call(x, pre)
            fc = got[2] if k == "step_forecast" else got
            T = 1 if k == "step_forecast" else x[1]
            given = ([x[4]] if x[4] is not None else None) if k == "step_forecast" else (row_keys(x[2], T) if x[3] else None)
            used: List[int] = []

            def hook(s, cloud, clock, obs_index, ts, ys, hs):
                key = int(given[s]) if given is not None else int(oracle.lib().oracle_c_derive_key(ref.seed, (1 << 63) | obs_index))
                used.append(key)
                if self.native:
                    self._forecast_row(fc, s, cloud, clock, ts, ys, hs, key, interval_of(x))
            ref.hook = hook
            try:
                exp = ref.apply(x)
            finally:
                ref.hook = None
            _eq("forecast keys", np.atleast_1d(np.asarray(fc["key"] if k == "step_forecast" else fc["keys"], dtype=np.uint64)),
                np.array(used, dtype=np.uint64))
            self._compare_return(x, got, exp)
            return
        if state_kind(x) is not None:
            pre = HostState.__new__(HostState); pre.__dict__.update(st.__dict__)
            exp = ref.apply(x)
            got = self._state_call(x, pre)
            self._compare_return(x, got, exp)
            return
        # ---- read-only
        ref.apply(x)
        if k == "summary":
            _compare_summary(call(g.summary, x[1]), ref.o.summary(x[1]))
        elif k == "particles":
            _eq("particles()", call(g.particles), ref.particles())
        elif k == "proposed":
            _eq("proposed()", call(g.proposed), ref.proposed())
        elif k == "ancestors":
            _eq("ancestors()", call(g.ancestors), ref.ancestors())
        elif k in ("weights", "logw"):
            self._compare_weights(asked=k)
        elif k == "observation_index":
            _eq("observation_index()", call(g.observation_index), st.obs)
        elif k == "forecast_key":
            if self.native:
                g.seed = ref.seed
            _eq("forecast_key()", call(g.forecast_key), ref.forecast_key())
        elif k == "last_device_us":
            if self.native:
                try:
                    us = _native_call(g.last_device_us)
                except Failed as e:
                    if e.code != ESTATE:
                        raise _Mismatch(f"last_device_us: status {e.code}")
                else:
                    if not (0.0 < us <= self.wall_us):
                        raise _Mismatch(f"last_device_us = {us} us; the run_more call it describes took {self.wall_us:.1f} us of wall time")
        elif k == "forecast":
            self._forecast(x)
        elif k == "forecast_posterior":
            self._forecast_posterior(x)
        else:
            raise AssertionError(f"unknown op {x!r}")

    def _compare_return(self, x: Op, got, exp):
        k = x.kind
        if k == "step":
            _eq("ll", got[0], exp[0]); _eq("ess", got[1], exp[1])
        elif k == "run":
            _eq("ll", got[0], exp[0]); _eq("ll_t", got[1], exp[1]); _eq("ess_t", got[2], exp[2])
            if x[3]:
                _eq("path", got[3], exp[3])
        elif k == "run_more":
            _eq("ll", got[0], exp[0]); _eq("ll_t", got[1], exp[1]); _eq("ess_t", got[2], exp[2])
        elif k == "interpolate":
            _eq("interpolate ll", got[0], exp[0])
            _compare_summary(got[1:], exp[1:], "interpolate")
        elif k in ("run_intervals", "run_intervals_more"):
            _eq("ll", got[0], exp[0]); _eq("ll_t", got[1], exp[1]); _eq("ess_t", got[2], exp[2])
            _compare_summary(got[3:9], exp[3:9], k + " rows")
        elif k == "step_intervals":
            _eq("ll", got[0], exp[0]); _eq("ess", got[1], exp[1])
            _compare_summary(got[2:8], exp[2:8], k + " row")
        elif k in ("run_forecasts", "run_forecasts_more"):
            _eq("ll", got["ll"], exp[0]); _eq("ll_t", got["ll_t"], exp[1]); _eq("ess_t", got["ess_t"], exp[2])
        elif k == "step_forecast":
            _eq("ll", got[0], exp[0]); _eq("ess", got[1], exp[1])
        elif k == "smooth":
            _eq("smooth ll", got[0], exp[0])
            _eq("smooth trajectories", got[7], exp[7])
            for q, name in ((2, "lower"), (3, "upper"), (5, "eta lower"), (6, "eta upper")):
                _eq("smooth " + name, got[q], exp[q])
            for q, name in ((1, "mean"), (4, "eta of mean")):
                try:
                    np.testing.assert_allclose(got[q], exp[q], rtol=1e-12, atol=0)    # (test_gpu_smooth.assert_equals_fleet: plain fp64 sums)
                except AssertionError as e:
                    raise _Mismatch(f"smooth {name}: {e}") from None
        elif k == "pmmh":
            for name, a, b in zip(("ll", "theta", "accepted", "last_state"), got, exp):
                _eq("pmmh " + name, a, b)
        elif k == "propagate":
            call = _native_call if self.native else (lambda f, *a, **kw: f(*a, **kw))
            _eq("proposed() after propagate", call(self.g.proposed), self.ref.o.proposed())
            if x[3] or self.spec.lgcp:
                _eq("logw() after propagate", call(self.g.logw), self.ref.o.logw())

    def _compare_weights(self, asked=None):
        """Whichever the handle keeps must equal what the oracle's log-weights give; the other getter must return CSSM_ESTATE; where
        the header lets the caller know which it is (ref.wmode), it must be that one."""
        g, ref = self.g, self.ref
        if not self.native:
            _eq("logw()", g.logw(), ref.o.logw())
            return
        w = _native_call(g.weights)                     # None: CSSM_ESTATE
        try:
            lw = _native_call(g.logw)
        except Failed as e:
            if e.code != ESTATE:
                raise _Mismatch(f"logw(): status {e.code}")
            lw = None
        if (w is None) == (lw is None):
            raise _Mismatch("weights() and logw() " + ("both refused" if w is None else "both answered") + ": exactly one of them is kept")
        mode = "w" if w is not None else "log"
        if ref.wmode is not None and mode != ref.wmode:
            raise _Mismatch(f"the handle keeps {'weights' if mode == 'w' else 'log-weights'}; after this sequence the header promises "
                            f"{'weights' if ref.wmode == 'w' else 'log-weights'}" + (f" (asked: {asked}())" if asked else ""))
        olw = ref.o.logw()
        if mode == "log":
            _eq("logw()", lw, olw)
        else:
            w1, c = w
            if c != ref.o.ref()[0]:
                raise _Mismatch(f"weights(): level {c!r}, oracle {ref.o.ref()[0]!r}")
            _eq("weights()", w1, oracle.c_exp(np.minimum(np.where(np.isnan(olw), -np.inf, olw) - c, 2.0 ** -20)))

    def _compare_cloud(self, what=""):
        ref, g = self.ref, self.g
        if ref.o is None or not ref.st.usable():
            return
        call = _native_call if self.native else (lambda f, *a, **kw: f(*a, **kw))
        _eq(what + "particles()", call(g.particles), ref.particles())
        _eq(what + "ancestors()", call(g.ancestors), ref.ancestors())
        if ref.st.weighted:
            self._compare_weights()

    def _forecast(self, x: Op):
        H, key, interval, cap = x[1], x[2], x[3], x[4]
        if not self.native:
            return
        from test_gpu_forecast import check_forecast, expected
        ref, g = self.ref, self.g
        times = horizon_times(ref.st.t, H)
        g.seed = ref.seed
        _native_call(g.set_option, OPT_FORECAST_CAP, cap)
        r = _native_call(g.forecast, times, key, interval, want_samples=self.n <= 5000)
        _native_call(g.set_option, OPT_FORECAST_CAP, 0)
        _eq("forecast key", r["key"], ref.forecast_key() if key is None else key)
        model = self.spec.model(ref.model_k)
        try:
            check_forecast(r, *expected(model, ref.particles(), ref.st.t, times, r["key"], self.twin), interval=interval)
        except AssertionError as e:
            raise _Mismatch(f"forecast: {e}") from None

    def _forecast_row(self, fc, s, cloud, clock, ts, ys, hs, key, interval):
        """Row s of a forecast call against test_gpu_forecast.expected from the cloud the reference has before that record; the PIT
        counts against numpy counts over the expected observation row (-1 for a record without a datum)."""
        from composablestatespacemodels_amd.filter import FORECAST_NAMES
        from test_gpu_forecast import check_forecast, expected
        model = self.spec.model(self.ref.model_k)
        states, etas, obs = expected(model, cloud, clock, [ts], key, self.twin)
        r = {name: np.asarray(fc[name])[s:s + 1] for name in FORECAST_NAMES}
        r["samples"] = None
        try:
            check_forecast(r, states, etas, obs, interval=interval)
        except AssertionError as e:
            raise _Mismatch(f"forecast row {s} (t = {ts!r}, key {key:#x}) is not the forecast of the cloud before that record: "
                            f"{str(e).strip() or 'an order statistic differs'}") from None
        below, equal = (int(np.sum(obs[0] < ys)), int(np.sum(obs[0] == ys))) if hs else (-1, -1)
        _eq(f"obs_below of row {s}", fc["obs_below"][s], below)
        _eq(f"obs_equal of row {s}", fc["obs_equal"][s], equal)

    def _forecast_posterior(self, x: Op):
        M, key = x[1], x[2]
        if not self.native:
            return
        from test_gpu_forecast import check_forecast
        from test_gpu_forecast_posterior import expected_posterior
        ref, g = self.ref, self.g
        model = self.spec.model(ref.model_k)
        p0 = Parameters([node for _, node, _ in model.leaves])
        th0 = np.asarray(p0.flattenParams())
        theta = th0 + 0.05 * np.cos(np.arange(M)[:, None] + np.arange(th0.size)[None, :])
        xs = 0.25 * np.sin(1.0 + np.arange(M)[:, None] + np.arange(g.d)[None, :])
        pick = (np.arange(self.n) * 7) % M
        times = horizon_times(2.0, 2)
        # (the handle lends its structure: NativePf.forecast_posterior hands the descriptor of ITS model)
        r = _native_call(g.forecast_posterior, theta, xs, 2.0, times, key, 0.975, pick=pick, want_samples=True)
        try:
            check_forecast(r, *expected_posterior(model, theta, xs, pick, 2.0, times, key, self.twin))
        except AssertionError as e:
            raise _Mismatch(f"forecast_posterior: {e}") from None

    # -- the whole sequence
    def run(self, seq: Sequence[Op]):
        pending_switch = False
        for i, x in enumerate(seq):
            try:
                self._do(x)
                cp, pending_switch = _is_checkpoint(x, i == len(seq) - 1, pending_switch)
                if cp:
                    self.ref.rebuild()
                    self._compare_cloud("checkpoint: ")
            except _Mismatch as e:
                raise Divergence(self._report(seq, i, str(e))) from None
            except Failed as e:
                raise Divergence(self._report(seq, i, f"a legal call returned status {e.code}")) from None

    def _report(self, seq, i, what) -> str:
        lines = [f"op {i} {seq[i]!r}: {what}   [{self.spec.name}, N = {self.n}, seed {self.seed}]",
                 "live prefix (model %d, key %d, resampler %d): %s" % (self.ref.base + (pasteable(self.ref.prefix),)) if self.ref.base else "no live prefix",
                 "sequence up to the diverging op:", pasteable(seq[:i + 1])]
        if self.make_subject is not None and self.ref.base and self.ref.o is not None and self.ref.prefix:
            # one extra run of what has just run cleanly on the reused handle, on a FRESH one: no retry of anything that failed
            try:
                k, seed, rs = self.ref.base
                fresh = self.make_subject(self.spec.model(k), seed)
                fresh.set_option(OPT_RESAMPLER, rs)
                sub = Runner(fresh, self.spec.name, self.n, seed, self.twin)
                sub.ref.model_k, sub.ref.seed, sub.ref.st.opts[OPT_RESAMPLER] = k, seed, rs
                sub.ref.st.model_k = k
                try:
                    sub.run(list(self.ref.prefix) + ([seq[i]] if state_kind(seq[i]) is None and seq[i].kind not in ILLEGAL_KINDS else []))
                    lines.insert(1, "a FRESH handle replaying the live prefix (default options) matches the oracle => stale state in the reused handle")
                except Divergence as e:
                    lines.insert(1, "a FRESH handle replaying the live prefix diverges too => a kernel or geometry bug, not stale state: " + str(e).split("\n")[0])
                fresh.close()
            except Failed as e:
                lines.insert(1, f"the fresh replay returned status {e.code}")
        return "\n".join(lines)


def run_sequence(subject, spec_name: str, n: int, seed: int, seq: Sequence[Op], twin=None, make_subject=None) -> Runner:
    check_legal(SPECS[spec_name], seq)
    r = Runner(subject, spec_name, n, seed, twin, make_subject)
    r.run(seq)
    return r
