"""``object Streaming`` of the reference (model/Streaming.scala): the pilot run that chooses the number of particles.

``pilotRun`` (:19-40) repeats ``llFilter`` under fixed parameters and reports the variance of the log-likelihood estimate per
particle count; the reference's advice is to pick the smallest N whose variance is about 1.  The repetitions of one N are
independent filters of the same data -- the R series of ONE fleet call (``NativePfFleet``) while a cloud fits a workgroup,
``NativePfBatch`` chains beyond that.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from . import _abi
from .filter import FilterFleet, NativePfBatch, NativePfFleet
from .model import Model, TimedObservation, split_data


class Streaming:
    @staticmethod
    def _lls(data, model: Model, n: int, keys: Sequence[int], device: int) -> np.ndarray:
        t, y, h = split_data(data)
        R = len(keys)
        if n <= _abi.FLEET_MAX_N:
            with NativePfFleet(model, n, R, device) as fl:
                fl.reseed(keys)
                ll, _, _, rc = fl.ll_filter([(t, y, h)] * R)
        else:
            ll, rc = np.zeros(R), np.zeros(R, dtype=np.int32)
            for g0 in range(0, R, 64):                      # (a batch holds at most 64 chains)
                ks = list(keys[g0:g0 + 64])
                b = NativePfBatch(model, n, len(ks), device)
                try:
                    ll[g0:g0 + len(ks)], _, rc[g0:g0 + len(ks)] = b.filter([model] * len(ks), ks, t, y, h, want_path=False)
                finally:
                    b.close()
        for r in range(R):
            if rc[r]:
                raise _abi.CssmError(int(rc[r]), f"pilot run: repetition {r} at {n} particles could not be weighed")
        return ll

    @staticmethod
    def pilotRun(data: Sequence[TimedObservation], model: Model, particles: Sequence[int], repetitions: int, seed: int = 20260101,
                 device: int = 0, ll_fn: Optional[Callable[[int, List[int]], Sequence[float]]] = None) -> List[Tuple[int, float]]:
        """``[(n, variance)]`` in the order of ``particles``: the unbiased variance (breeze ``variance``: divisor R - 1) of the
        ``repetitions`` log-likelihoods of ``llFilter`` at n particles, repetition r under the key ``cssm_pf_run_key(seed, r)``.
        ``ll_fn(n, keys)`` replaces the filter runs (tests)."""
        if repetitions < 2:
            raise ValueError("the variance needs at least two repetitions")
        keys = FilterFleet.keys(seed, repetitions)
        out = []
        for n in particles:
            lls = np.asarray(ll_fn(int(n), keys) if ll_fn is not None else Streaming._lls(data, model, int(n), keys, device), dtype=np.float64)
            if lls.shape != (repetitions,):
                raise ValueError("one log-likelihood per repetition")
            out.append((int(n), float(np.var(lls, ddof=1))))
        return out
