"""Maximum likelihood by iterated filtering on a fleet (``cssm_fleet_if2``).  An EXTENSION: the reference has no likelihood maximiser --
``examples/DetermineParameters.scala`` assumes the starting value of its chains.  This is IF2 of Ionides, Nguyen, Atchade, Stoev and King
(PNAS 2015), the ``mif2`` of the R package pomp: every particle carries its own parameter vector, which random-walks with a shrinking step
and is resampled together with the state; after a few dozen passes over the data the swarm sits at the maximum of the likelihood.  Usual
practice is many searches from many starting points: here S searches, a series of a fleet each, all iterations in one launch.

Marshalling only: the search is the library's (include/cssm_pf.h; its arithmetic is part of the numerics contract)."""
from typing import List, Optional, Sequence

import numpy as np

from . import _abi
from .filter import NativePf, NativePfFleet
from .model import Parameters, UnparamModel
from .pmmh import pmmh_fleet_pack


class If2Result:
    """``theta_mean[S, iters, n_theta]``: the swarm's mean per stored parameter after each iteration; ``ll[S, iters]``: the perturbed
    filter's log-likelihood estimate (a diagnostic, not the likelihood at the mean); ``rc[S]``: a search's own status (-5: some record
    left none of its particles a usable weight; its rows read NaN from that iteration on); ``swarm[S, n_theta, N]``: the final swarm
    (``IF2(..., swarm0=result.swarm, first_iter=iters)`` continues the search)."""

    def __init__(self, starts: Sequence[Parameters], out: dict):
        self._starts = list(starts)
        self.theta_mean, self.ll, self.rc, self.swarm = out["theta_mean"], out["ll"], out["rc"], out["swarm"]

    def parameters(self, k: int) -> Parameters:
        """The final swarm mean of search k as a Parameters tree (stored, i.e. unconstrained, values)."""
        return self._starts[k].withFlat([float(v) for v in self.theta_mean[k, -1]])


def IF2(unparam: UnparamModel, starts: Sequence[Parameters], datas, n: int, rw_sd, cooling: float, iters: int, seeds: Sequence[int],
        device: int = 0, fleet: Optional[NativePfFleet] = None, swarm0=None, first_iter: int = 0, iters_per_launch: int = 0) -> If2Result:
    """``len(starts)`` searches, search k from ``starts[k]`` under ``seeds[k]`` with ``n`` particles.  ``datas``: one data set (every search
    sees it) or one per search.  ``rw_sd``: the random-walk standard deviation per stored parameter in ``flattenParams`` order (0 keeps a
    parameter fixed), at iteration 0; ``cooling``: the factor it shrinks by over 50 iterations, in (0, 1]."""
    S = len(starts)
    if S < 1 or len(seeds) != S:
        raise ValueError("one seed per search")
    theta0 = np.ascontiguousarray([p.flattenParams() for p in starts], dtype=np.float64)
    off, t, y, has = pmmh_fleet_pack(datas, S)
    model = unparam.run(starts[0])
    own = fleet is None
    if own:
        fleet = NativePfFleet(model, n, S, device)
    elif fleet.S != S or fleet.n != int(n):
        raise ValueError(f"the fleet holds {fleet.S} series of {fleet.n} particles, the searches need {S} of {n}")
    try:
        split: List = [(t[a:b], y[a:b], has[a:b]) for a, b in zip(off[:-1].tolist(), off[1:].tolist())]
        out = fleet.if2(model.descriptor(), split, rw_sd, cooling, iters, seeds, theta0=theta0, swarm0=swarm0, first_iter=first_iter,
                        iters_per_launch=iters_per_launch, want_swarm=True)
    finally:
        if own:
            fleet.close()
    return If2Result(starts, out)


def IF2Single(unparam: UnparamModel, start: Parameters, data, n: int, rw_sd, cooling: float, iters: int, seed: int, device: int = 0,
              handle: Optional[NativePf] = None, swarm0=None, first_iter: int = 0) -> If2Result:
    """One search with ``n`` particles on a single handle (``cssm_pf_if2``): the swarm is tiled over many workgroups, so ``n`` is not bound
    by a fleet's 4096 -- the point estimate a PMMH chain at N = 100 000 should start from.  Arguments as ``IF2``'s, for one search; the
    result is shaped as one search (S = 1), so ``.parameters(0)`` is the final mean.  ``handle``: a ``NativePf`` of the model's structure
    and ``n`` particles to lend (its cloud, clock and key stay what they were)."""
    off, t, y, has = pmmh_fleet_pack(data, 1)
    theta0 = np.ascontiguousarray(start.flattenParams(), dtype=np.float64)
    own = handle is None
    if own:
        handle = NativePf(unparam.run(start), n, int(seed), device)
    elif handle.n != int(n):
        raise ValueError(f"the handle holds {handle.n} particles, the search needs {n}")
    try:
        a, b = int(off[0]), int(off[1])
        one = handle.if2(t[a:b], y[a:b], has[a:b], rw_sd, cooling, iters, seed, theta0=theta0, swarm0=swarm0, first_iter=first_iter,
                         want_swarm=True)
    finally:
        if own:
            handle.close()
    out = {"theta_mean": one["theta_mean"][None], "ll": one["ll"][None], "rc": np.asarray([one["rc"]], dtype=np.int32),
           "swarm": one["swarm"][None]}
    return If2Result([start], out)
