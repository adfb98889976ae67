"""SMC2: online parameter learning over two fleets (EXTENSION -- the reference has no online parameter learner; its
``ParamFilterState(t, observation, params, state, ll)``, model/ParticleFilter.scala:89-94, is never used).

Chopin, Jacob and Papaspiliopoulos (2013): S parameter particles, each with a bootstrap filter of N state particles.  A fleet already is
that structure -- one launch advances every series by an observation and returns its likelihood increment, the weight of that parameter
particle.  What the driver adds is the parameter level, in plain numpy, and two device operations: when the parameter particles are
resampled the cloud of series ``a[k]`` becomes the cloud of series ``k`` (``NativePfFleet.copy_series``), and when a PMMH rejuvenation
move is accepted the freshly filtered cloud of a proposal fleet replaces the series' cloud (``copy_series(..., src=B)``).

The driver talks to an ENGINE (``FleetEngine`` below; any object with its eight methods), and everything random at the parameter level
comes from numpy: the same driver over another engine with the same filter bits (the CPU oracle in the tests) agrees bit for bit.

The algorithm, exactly:

* State: ``theta[S, n_theta]`` in ``flattenParams`` order, ``logw[S] = 0``, ``ll_run[S] = 0``, ``log_evidence = 0``, a generation counter
  ``g = 0``, the observations seen so far.
* First observation: parameters set, keys set to ``cssm_pf_run_key(seed, k)``, every series initialised at the observation's own time (as
  ``llFilter`` does with ``t0 = min t``: observations arrive in time order); then it is treated like any other.
* Each observation: one engine step of the live series gives ``ll_new``; ``inc = ll_new - ll_run`` (0 for an observation without a datum).
  A series whose step is ``CSSM_ENONFINITE`` gets ``inc = -inf`` and is masked out of later steps until a resampling replaces it; if every
  series is dead the step raises.  ``log_evidence += lse(logw + inc) - lse(logw)``; ``logw += inc``; ``ESS = exp(2 lse(logw) - lse(2 logw))``.
* Rejuvenation, when ``ESS < ess_fraction * S``:
  1. the weighted mean and covariance of ``theta[:, free]`` BEFORE resampling; ``L = chol(scale^2 cov + 1e-12 I)``, ``scale`` defaulting to
     ``2.38 / sqrt(len(free))``;
  2. systematic ancestors ``anc`` of the normalised weights under ONE uniform (a numpy statement here, not the device seam: the CPU twin
     runs without a GPU); ``engine.clone(anc)``; ``theta, ll_run <- [anc]``; ``logw = 0``;
  3. ``moves`` rounds: ``theta' = theta + L z`` on the free components; ``engine.propose`` filters the whole prefix afresh under ``theta'``
     on the proposal fleet, a fresh key per series; accept where the filter succeeded and
     ``log u < ll' + log_prior(theta') - ll_run - log_prior(theta)``; ``engine.adopt(accepted)``.  A ``theta'`` that ``unparam.run`` or
     the descriptor refuses, or that is not finite, is rejected (its series filters its current parameters and the result is ignored);
  4. ``g += 1`` and every series of the running fleet gets the fresh key of the new generation (``engine.reseed(keys)``).
* The arithmetic of the two recurrences: between two resamplings ``logw`` telescopes to ``ll_run - (ll_run where logw was last 0)`` and
  ``log_evidence`` to ``(its value there) + lse(logw) - log S``; the driver evaluates these closed forms, not the running sums, so that
  without rejuvenation ``logw`` IS the filters' log-likelihood and ``log_evidence = lse(ll) - log S`` to the bit.
* Randomness: ONE ``np.random.Generator(np.random.PCG64(seed))``; per rejuvenation, in this order: the resampling uniform
  (``random()``), then per round ``z = standard_normal((S, len(free)))`` and ``u = random(S)``.  Nothing else draws from it.
* Key streams: every Philox key is ``cssm_pf_run_key(seed, c)`` with a counter ``c`` that is never reused:
  ``c = (g (moves + 1) + slot) S + k`` for series k -- slot 0: the RUNNING fleet's keys of generation g (g = 0: the initial keys ``c = k``);
  slot r = 1 .. moves: the PROPOSAL fleet's keys in round r of the rejuvenation that ends generation g.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from . import _abi
from .model import Model, Parameters, TimedObservation, UnparamModel

__all__ = ["SMC2", "Smc2State", "FleetEngine", "logsumexp", "systematic_ancestors"]


def logsumexp(a) -> float:
    """log sum exp of a vector that may hold -inf entries (all -inf: -inf)."""
    a = np.asarray(a, dtype=np.float64)
    m = float(np.max(a))
    if m == -np.inf:
        return -np.inf
    return m + float(np.log(np.sum(np.exp(a - m))))


def systematic_ancestors(w, u: float) -> np.ndarray:
    """Systematic ancestors of normalised weights ``w`` under one uniform ``u``: position ``(u + i) / S`` falls into the ancestor whose
    cumulative weight first exceeds it (a weight of zero is never chosen)."""
    S = len(w)
    cum = np.cumsum(w)
    cum[-1] = 1.0
    return np.minimum(np.searchsorted(cum, (u + np.arange(S)) / S, side="right"), S - 1).astype(np.int64)


@dataclass
class Smc2State:
    t: float
    theta: np.ndarray          # [S, n_theta], flattenParams order
    logw: np.ndarray           # [S], unnormalised
    ess: float
    log_evidence: float        # log p(y_1 .. y_t), accumulated
    resampled: bool
    accepted: int              # moves accepted in this step's rejuvenation (0 without one), over all rounds


class FleetEngine:
    """The shipped engine: two ``NativePfFleet`` of S series and N particles -- A runs, B filters proposals.

    The protocol an engine serves (``models``: S parameterised ``Model``; ``keys``: S Philox keys; ``data``: ``(t, y, has)`` arrays):
    ``init(models, keys, t0)``; ``step(t, y, has, active) -> (ll[S], rc[S])`` (ll accumulated, rc -5 where the weights were unusable);
    ``clone(anc)`` (series k <- series anc[k], simultaneously, each keeping its own key); ``propose(models, keys, data) -> (ll[S], ok[S])``
    (a fresh filter of the whole prefix per series on the proposal side); ``adopt(accepted)`` (the proposal's filter replaces the
    series' where accepted); ``reseed(keys)`` (every running series gets a new key; its cloud stays); ``summary(interval)``; ``close()``."""

    def __init__(self, model: Model, n: int, series: int, device: int = 0):
        from .filter import NativePfFleet
        self.A = NativePfFleet(model, n, series, device)
        self.B = NativePfFleet(model, n, series, device)
        self.S = int(series)

    def init(self, models: Sequence[Model], keys: Sequence[int], t0: float):
        self.A.set_params(models)
        self.A.reseed(keys)
        self.A.init(float(t0))

    def step(self, t: float, y: float, has: bool, active) -> Tuple[np.ndarray, np.ndarray]:
        S = self.S
        ll, _, rc = self.A.step(np.full(S, float(t)), np.full(S, float(y)), has=np.full(S, 1 if has else 0, dtype=np.uint8), active=active)
        return ll, rc

    def clone(self, anc):
        rc = self.A.copy_series(anc)
        if rc.any():
            raise RuntimeError(f"SMC2: resampling chose a series without a cloud (rc {rc.tolist()})")

    def propose(self, models: Sequence[Model], keys: Sequence[int], data) -> Tuple[np.ndarray, np.ndarray]:
        self.B.set_params(models)
        self.B.reseed(keys)
        ll, _, _, rc = self.B.ll_filter_packed(*self.B.pack([data] * self.S))
        return ll, rc == 0

    def adopt(self, accepted):
        if np.any(accepted):
            rc = self.A.copy_series([k if a else -1 for k, a in enumerate(accepted)], src=self.B)
            if rc.any():
                raise RuntimeError(f"SMC2: an accepted proposal has no cloud (rc {rc.tolist()})")

    def reseed(self, keys: Sequence[int]):
        self.A.reseed(keys)

    def summary(self, interval: float = 0.975):
        return self.A.summary(interval)

    def close(self):
        self.A.close()
        self.B.close()


class SMC2:
    """``SMC2(unparam, prior_draws, n)``: S = ``len(prior_draws)`` parameter particles drawn by the caller from a PROPER prior (the
    library's PMMH is flat-prior; SMC2 needs a proper start), N = ``n`` state particles each.  ``log_prior`` acts on the flat
    unconstrained vector (default 0); ``free`` selects the components of it that move (default all).  See the module docstring for the
    algorithm, the order of the random draws and the key streams."""

    def __init__(self, unparam: UnparamModel, prior_draws: Sequence[Parameters], n: int, log_prior: Optional[Callable] = None,
                 free: Optional[Sequence[int]] = None, ess_fraction: float = 0.5, moves: int = 1, scale: Optional[float] = None,
                 seed: int = 20260101, device: int = 0, engine=None):
        if len(prior_draws) < 1:
            raise ValueError("SMC2 needs at least one parameter particle")
        self.unparam, self.template = unparam, prior_draws[0]
        self.S, self.n = len(prior_draws), int(n)
        self.theta = np.ascontiguousarray([p.flattenParams() for p in prior_draws], dtype=np.float64)
        self.n_theta = self.theta.shape[1]
        self.free = np.arange(self.n_theta) if free is None else np.asarray(list(free), dtype=np.int64)
        if len(self.free) < 1 or (self.free < 0).any() or (self.free >= self.n_theta).any() or len(set(self.free.tolist())) != len(self.free):
            raise ValueError(f"free must name distinct components of the flat vector (0 .. {self.n_theta - 1})")
        if int(moves) < 0:
            raise ValueError("moves must not be negative")
        self.log_prior = log_prior if log_prior is not None else (lambda th: 0.0)
        self.ess_fraction, self.moves = float(ess_fraction), int(moves)
        self.scale = 2.38 / np.sqrt(len(self.free)) if scale is None else float(scale)
        self.seed = int(seed)
        self.rng = np.random.Generator(np.random.PCG64(self.seed))
        self.lib = _abi.load_library()
        self.models: List[Model] = [unparam.run(p) for p in prior_draws]
        self.engine = engine if engine is not None else FleetEngine(self.models[0], self.n, self.S, device)
        self.logw = np.zeros(self.S)
        self.ll_run = np.zeros(self.S)
        self.lp = np.array([float(self.log_prior(th)) for th in self.theta])
        self.active = np.ones(self.S, dtype=bool)
        self.log_evidence = 0.0
        self.ll_base = np.zeros(self.S)            # ll_run where logw was last 0: at the start, behind the last rejuvenation
        self.ev_base = 0.0                         # log_evidence at that point
        self.g = 0
        self.seen: List[TimedObservation] = []
        self.rejuvenations = 0

    # -- keys
    def _keys(self, slot: int) -> List[int]:
        base = (self.g * (self.moves + 1) + slot) * self.S
        return [int(self.lib.cssm_pf_run_key(self.seed, base + k)) for k in range(self.S)]

    # -- a proposal's model, or None where unparam.run or the descriptor refuses it
    def _model_of(self, th) -> Optional[Model]:
        if not np.all(np.isfinite(th)):
            return None
        try:
            model = self.unparam.run(self.template.withFlat(th))
            desc = model.descriptor()
        except (ValueError, OverflowError, ArithmeticError):
            return None
        words, d = (C.c_uint32 * (_abi.MAX_DIM // 4))(), C.c_int32()
        return model if self.lib.cssm_model_structure(desc.ptr(), words, C.byref(d)) == 0 else None

    def _data(self):
        t = np.array([o.t for o in self.seen], dtype=np.float64)
        y = np.array([0.0 if o.observation is None else o.observation for o in self.seen], dtype=np.float64)
        has = np.array([0 if o.observation is None else 1 for o in self.seen], dtype=np.uint8)
        return t, y, has

    def step(self, obs: TimedObservation) -> Smc2State:
        S = self.S
        if not self.seen:
            self.engine.init(self.models, self._keys(0), obs.t)
        self.seen.append(obs)
        has = obs.observation is not None
        ll_new, rc = self.engine.step(obs.t, 0.0 if not has else obs.observation, has, self.active.astype(np.uint8))
        for k in range(S):
            if not self.active[k]:
                continue
            if rc[k] == _abi.CSSM_ENONFINITE:
                self.active[k] = False                     # inc = -inf: masked until a resampling replaces it
            elif rc[k] != 0:
                raise _abi.CssmError(int(rc[k]), f"SMC2: series {k} could not be stepped")
            else:
                self.ll_run[k] = ll_new[k]                 # (an observation without a datum leaves it as it was: inc = 0)
        if not self.active.any():
            raise RuntimeError(f"SMC2: every parameter particle is dead at t = {obs.t} (no series could weigh the observation)")
        # the recurrences in closed form since the last resampling (see the module docstring)
        self.logw = np.where(self.active, self.ll_run - self.ll_base, -np.inf)
        self.log_evidence = self.ev_base + (logsumexp(self.logw) - float(np.log(S)))
        ess = float(np.exp(2.0 * logsumexp(self.logw) - logsumexp(2.0 * self.logw)))
        resampled, accepted = False, 0
        if ess < self.ess_fraction * S:
            resampled, accepted = True, self._rejuvenate()
        return Smc2State(float(obs.t), self.theta.copy(), self.logw.copy(), ess, float(self.log_evidence), resampled, accepted)

    def _rejuvenate(self) -> int:
        S, free = self.S, self.free
        w = np.exp(self.logw - np.max(self.logw))
        w = w / np.sum(w)
        x = self.theta[:, free]
        mean = w @ x
        dev = x - mean
        cov = (dev * w[:, None]).T @ dev
        L = np.linalg.cholesky(self.scale ** 2 * cov + 1e-12 * np.eye(len(free)))
        anc = systematic_ancestors(w, float(self.rng.random()))
        self.engine.clone(anc)
        self.theta, self.ll_run, self.lp = self.theta[anc].copy(), self.ll_run[anc].copy(), self.lp[anc].copy()
        self.models = [self.models[int(a)] for a in anc]
        self.logw = np.zeros(S)
        self.active[:] = True
        data = self._data()
        accepted = 0
        for r in range(1, self.moves + 1):
            z = self.rng.standard_normal((S, len(free)))
            u = self.rng.random(S)
            prop = self.theta.copy()
            prop[:, free] += z @ L.T
            built = [self._model_of(th) for th in prop]
            valid = np.array([m is not None for m in built])
            ll_p, ok = self.engine.propose([m if m is not None else self.models[k] for k, m in enumerate(built)], self._keys(r), data)
            lp_p = np.array([float(self.log_prior(th)) if v else -np.inf for th, v in zip(prop, valid)])
            with np.errstate(invalid="ignore", divide="ignore"):
                acc = valid & np.asarray(ok, dtype=bool) & (np.log(u) < ll_p + lp_p - self.ll_run - self.lp)
            self.engine.adopt(acc)
            for k in np.flatnonzero(acc):
                self.theta[k], self.ll_run[k], self.lp[k], self.models[k] = prop[k], ll_p[k], lp_p[k], built[k]
            accepted += int(acc.sum())
        self.ll_base, self.ev_base = self.ll_run.copy(), self.log_evidence
        self.g += 1
        self.engine.reseed(self._keys(0))   # (g is the new generation: its running keys)
        self.rejuvenations += 1
        return accepted

    def run(self, data: Sequence[TimedObservation]) -> List[Smc2State]:
        return [self.step(o) for o in data]

    def posterior(self) -> Tuple[np.ndarray, np.ndarray]:
        """``(theta[S, n_theta], weights[S])``: the parameter particles and their normalised weights."""
        w = np.exp(self.logw - np.max(self.logw))
        return self.theta.copy(), w / np.sum(w)

    def close(self):
        self.engine.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
