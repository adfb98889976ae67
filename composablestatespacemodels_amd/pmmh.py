"""Host-side mirror of the reference's PMMH surface (model/PMMH.scala, model/MarkovChain.scala).

The MCMC chain is sequential and stays on the host (BASELINE.json north star); each iteration's
work is one native filter run.  Two entry points:

* ``MetropolisHastings.pmmhState(initP, proposal, logTransition, prior)(pf)`` -- the generic
  reference signature (PMMH.scala:161-167): ``pf`` is a ``BootstrapFilter`` (package.scala:24), i.e.
  a callable ``params -> (ll, path)``; ``proposal(params, rng)`` draws a proposal.  Returns an
  iterator of ``MetropState`` (the stream drops the initial state, PMMH.scala:97).
* ``pmmh_native`` -- the wiring of examples/DetermineParameters.scala:58-80 (``perturb(delta)``
  proposal, symmetric transition, flat prior) executed by ``cssm_pmmh_run`` inside the library with
  the contract's Philox streams, so a CPU restatement reproduces the chain bit for bit.
* ``pmmh_fleet_chains`` -- whole chains on the device (``cssm_fleet_pmmh_chains``), a chain per series of a fleet, with the reference's
  ``prior`` argument (``Prior``, ``priors_for``) and its tuned proposal ``Parameters.perturbMvn(chol)`` (``covariance``,
  ``chol_from_pilot``; ``perturbMvn`` / ``perturbMvnEigen`` are the same proposals for the generic loop above).
* ``pmmh_lgcp_fleet_chains`` -- the same for log-Gaussian Cox processes (``cssm_fleet_pmmh_chains_lgcp``): a chain per event stream of
  an LGCP fleet.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Callable, Iterator, Optional, Sequence, Tuple

import numpy as np

from . import _abi
from .filter import NativeLgcpFleet, NativePf, NativePfFleet, Resampling
from .model import Parameters, UnparamModel, split_data


@dataclass
class MetropState:  # PMMH.scala:10-14
    ll: float
    params: Parameters
    sde: object
    accepted: int


@dataclass
class ParamsState:  # PMMH.scala:17 (what `params` emits: the chain without the sampled state)
    ll: float
    params: Parameters
    accepted: int


class ParametersProposal:
    """``Parameters.perturb(delta)`` (Parameters.scala:65-67): independent Gaussian(theta_k, sqrt(delta))
    on every stored scalar, scale included."""

    def __init__(self, delta: float):
        self.sd = math.sqrt(delta)

    def __call__(self, p: Parameters, rng: np.random.Generator) -> Parameters:
        theta = np.asarray(p.flattenParams())
        return p.withFlat(theta + self.sd * rng.standard_normal(theta.size))


class MetropolisHastings:
    @staticmethod
    def mhStep(s: MetropState, proposal, logTransition, prior, pf, rng) -> MetropState:
        """PMMH.scala:68-81; the stored ll of the current state is reused, not re-estimated (:63-66)."""
        prop = proposal(s.params, rng)
        ll, path = pf(prop)
        a = ll + logTransition(prop, s.params) + prior(prop) - logTransition(s.params, prop) - s.ll - prior(s.params)
        u = rng.random()
        if math.log(u) < a if u > 0.0 else True:
            return MetropState(ll, prop, path[-1] if len(path) else None, s.accepted + 1)
        return s

    @staticmethod
    def pmmhState(initP: Parameters, proposal, logTransition, prior):
        def run(pf: Callable[[Parameters], Tuple[float, Sequence]], rng: Optional[np.random.Generator] = None,
                iters: Optional[int] = None) -> Iterator[MetropState]:
            rng = rng or np.random.default_rng()
            s = MetropState(-1e99, initP, None, 0)      # PMMH.scala:121
            k = 0
            while iters is None or k < iters:
                s = MetropolisHastings.mhStep(s, proposal, logTransition, prior, pf, rng)
                k += 1
                yield s
        return run


    @staticmethod
    def approxMhStep(s: MetropState, proposal, logTransition, prior, pf, rng) -> MetropState:
        """ApproxPMMH.mhStep (PMMH.scala:138-152): the likelihood of the CURRENT parameters is estimated again in every
        step (two filter runs per iteration: the proposal's first, then the current one's), and a rejected step carries
        that fresh estimate and its last sampled state."""
        prop = proposal(s.params, rng)
        ll, path = pf(prop)
        old_ll, old_path = pf(s.params)
        a = ll + logTransition(prop, s.params) + prior(prop) - logTransition(s.params, prop) - old_ll - prior(s.params)
        u = rng.random()
        if math.log(u) < a if u > 0.0 else True:
            return MetropState(ll, prop, path[-1] if len(path) else None, s.accepted + 1)
        return MetropState(old_ll, s.params, old_path[-1] if len(old_path) else None, s.accepted)

    @staticmethod
    def approxPmmh(initP: Parameters, proposal, logTransition, prior):
        """MetropolisHastings.approxPmmh (PMMH.scala:169-175): as pmmhState with ApproxPMMH's step."""
        def run(pf: Callable[[Parameters], Tuple[float, Sequence]], rng: Optional[np.random.Generator] = None,
                iters: Optional[int] = None) -> Iterator[MetropState]:
            rng = rng or np.random.default_rng()
            s = MetropState(-1e99, initP, None, 0)      # PMMH.scala:135
            k = 0
            while iters is None or k < iters:
                s = MetropolisHastings.approxMhStep(s, proposal, logTransition, prior, pf, rng)
                k += 1
                yield s
        return run

    @staticmethod
    def params(chain: Iterator[MetropState]) -> Iterator[ParamsState]:
        """MetropolisHastings.params (PMMH.scala:89-93): the chain's (ll, params, accepted)."""
        for s in chain:
            yield ParamsState(s.ll, s.params, s.accepted)

    @staticmethod
    def pmmhStep(pos: Callable, proposal: Callable, s: Tuple[float, object], rng) -> Tuple[float, object]:
        """MetropolisHastings.pmmhStep (PMMH.scala:177-191): Metropolis step on a (log-posterior, parameter) pair with a
        symmetric proposal; `pos` returns the log-posterior estimate of a proposal."""
        prop = proposal(s[1], rng)
        ll = pos(prop)
        u = rng.random()
        return (ll, prop) if (u <= 0.0 or math.log(u) < ll - s[0]) else s


def bootstrap_filter(unparam: UnparamModel, data, n: int, seed: int = 20260101, device: int = 0):
    """``Reader { p => Filter(model.run(p).get, resample).filter(data, n) }`` on one native handle
    (examples/DetermineParameters.scala:70-72): re-parameterised per call, never re-allocated."""
    t, y, h = split_data(data)
    state = {"pf": None, "calls": 0}

    def pf(p: Parameters):
        model = unparam.run(p)
        if state["pf"] is None:
            state["pf"] = NativePf(model, n, seed, device)
        else:
            state["pf"].set_params(model)
        state["pf"].reseed(state["pf"].lib.cssm_pf_run_key(seed & (2**64 - 1), 1 + state["calls"]))   # a PRF of (seed, call), never seed + call
        state["calls"] += 1
        ll, _, _, path = state["pf"].run(t, y, h, want_path=True)
        return ll, path
    return pf


def pmmh_native(unparam: UnparamModel, init: Parameters, data, n: int, delta: float, iters: int,
                seed: int = 20260101, device: int = 0):
    """Returns (ll[iters], theta[iters, n_theta], accepted[iters], last_state[iters, d])."""
    t, y, h = split_data(data)
    model = unparam.run(init)
    pf = NativePf(model, n, seed, device)
    theta0 = np.ascontiguousarray(init.flattenParams(), dtype=np.float64)
    nt = theta0.size
    ll = np.zeros(iters); th = np.zeros((iters, nt)); acc = np.zeros(iters, dtype=np.int32); last = np.zeros((iters, pf.d))
    dp = C.POINTER(C.c_double)
    desc = model.descriptor()
    rc = pf.lib.cssm_pmmh_run(pf._h, desc.ptr(), theta0.ctypes.data_as(dp), nt, float(delta), t.ctypes.data_as(dp),
                              y.ctypes.data_as(dp), h.ctypes.data_as(C.POINTER(C.c_uint8)), len(t), int(seed), int(iters),
                              ll.ctypes.data_as(dp), th.ctypes.data_as(dp), acc.ctypes.data_as(C.POINTER(C.c_int32)),
                              last.ctypes.data_as(dp))
    pf.close()
    _abi.check(rc)
    return ll, th, acc, last


def pmmh_native_batched(unparam: UnparamModel, inits: Sequence[Parameters], data, n: int, delta: float, iters: int,
                        seeds: Sequence[int], device: int = 0):
    """``len(inits)`` chains in lockstep (``cssm_pmmh_run_batched``): chain k is ``pmmh_native(unparam, inits[k], ..., seed=seeds[k])`` bit
    for bit -- what examples/DetermineParameters.scala:68-69 runs as two chains under ``mapAsync(2)`` -- but every iteration's filters
    of all chains run as ONE batch on the GPU.  Returns (ll[B, iters], theta[B, iters, n_theta], accepted[B, iters], last_state[B, iters, d])."""
    t, y, h = split_data(data)
    B = len(inits)
    if B < 1 or len(seeds) != B:
        raise ValueError("one seed per chain")
    model = unparam.run(inits[0])
    desc = model.descriptor()
    lib = _abi.load_library()
    hb = C.c_void_p()
    _abi.check(lib.cssm_pfb_create(desc.ptr(), int(n), B, int(device), C.byref(hb)))
    try:
        d = int(lib.cssm_pf_dim(lib.cssm_pfb_chain(hb, 0)))
        theta0 = np.ascontiguousarray([p.flattenParams() for p in inits], dtype=np.float64)
        nt = theta0.shape[1]
        ll = np.zeros((B, iters)); th = np.zeros((B, iters, nt)); acc = np.zeros((B, iters), dtype=np.int32); last = np.zeros((B, iters, d))
        sd = np.ascontiguousarray([int(x) & (2**64 - 1) for x in seeds], dtype=np.uint64)
        dp = C.POINTER(C.c_double)
        _abi.check(lib.cssm_pmmh_run_batched(hb, desc.ptr(), theta0.ctypes.data_as(dp), nt, float(delta), t.ctypes.data_as(dp), y.ctypes.data_as(dp),
                                             h.ctypes.data_as(C.POINTER(C.c_uint8)), len(t), sd.ctypes.data_as(C.POINTER(C.c_uint64)), int(iters),
                                             ll.ctypes.data_as(dp), th.ctypes.data_as(dp), acc.ctypes.data_as(C.POINTER(C.c_int32)), last.ctypes.data_as(dp)))
    finally:
        lib.cssm_pfb_destroy(hb)
    return ll, th, acc, last


def pmmh_fleet_pack(datas, chains: int):
    """The ragged arrays of ``cssm_fleet_pmmh_run`` for ``chains`` chains: ``datas`` is ONE data set (a sequence of TimedObservation: every
    chain sees it) or a sequence of ``chains`` data sets.  Refuses an empty data set here, before any device call."""
    datas = list(datas)
    shared = len(datas) == 0 or hasattr(datas[0], "observation")
    if shared:
        datas = [datas] * chains
    if len(datas) != chains:
        raise ValueError(f"one data set, or one per chain ({chains}), not {len(datas)}")
    cache = {}
    split = []
    for k, d in enumerate(datas):
        if len(d) == 0:
            raise ValueError(f"chain {k} has an empty data set (the reference's minBy throws on an empty Vector)")
        split.append(cache.setdefault(id(d), split_data(d)))
    return NativePfFleet.pack(split)


def pmmh_native_fleet(unparam: UnparamModel, inits: Sequence[Parameters], datas, n: int, delta: float, iters: int,
                      seeds: Sequence[int], device: int = 0, fleet: Optional[NativePfFleet] = None):
    """``len(inits)`` chains in lockstep on a fleet (``cssm_fleet_pmmh_run``), a chain per series and ONE launch per iteration: chain k is
    ``pmmh_native(unparam, inits[k], data_k, n, delta, iters, seed=seeds[k])`` bit for bit.  ``datas``: one data set (every chain sees it)
    or a sequence of S data sets (a chain per sensor).  For the reference's everyday cloud sizes (n <= ``_abi.FLEET_MAX_N``, no LGCP,
    systematic resampling); ``pmmh_native_batched`` serves the rest.  ``fleet``: a NativePfFleet of S series and n particles to reuse.
    Returns (ll[S, iters], theta[S, iters, n_theta], accepted[S, iters], last_state[S, iters, d]); each chain's rows go through
    ``posterior_rows`` unchanged."""
    S = len(inits)
    if S < 1 or len(seeds) != S:
        raise ValueError("one seed per chain")
    theta0 = [np.asarray(p.flattenParams(), dtype=np.float64) for p in inits]
    if any(th.shape != theta0[0].shape for th in theta0):
        raise ValueError("every chain's initial parameters must flatten to the same length")
    theta0 = np.ascontiguousarray(theta0, dtype=np.float64)
    off, t, y, has = pmmh_fleet_pack(datas, S)
    model = unparam.run(inits[0])
    desc = model.descriptor()
    own = fleet is None
    if own:
        try:
            fleet = NativePfFleet(model, n, S, device)
        except _abi.CssmError as e:
            if e.code in (_abi.CSSM_EINVAL_ARG, _abi.CSSM_EINVAL_DESC):
                raise _abi.CssmError(e.code, f"{e.args[0]}; cssm_pmmh_run_batched (pmmh_native_batched) serves the chains a fleet does not") from None
            raise
    elif fleet.S != S or fleet.n != int(n):
        raise ValueError(f"the fleet holds {fleet.S} series of {fleet.n} particles, the run needs {S} of {n}")
    try:
        return fleet.pmmh_run(desc, theta0, delta, off, t, y, has, seeds, iters)
    finally:
        if own:
            fleet.close()


class Prior:
    """A slot's prior on the STORED (unconstrained) value, as ``cssm_fleet_pmmh_chains`` takes it (``cssm_prior``): the reference's
    ``prior: P => LogLikelihood`` (PMMH.scala:32,72-73) as a sum of independent terms over the flattened parameters."""

    @staticmethod
    def flat() -> _abi.Prior:
        return _abi.Prior(_abi.CSSM_PRIOR_FLAT, 0, 0.0, 0.0)

    @staticmethod
    def normal(mean: float, sd: float) -> _abi.Prior:
        """``-(z z) / 2``, ``z = (theta - mean) / sd`` (constants dropped: only differences decide)."""
        return _abi.Prior(_abi.CSSM_PRIOR_NORMAL, 0, float(mean), float(sd))

    @staticmethod
    def uniform(lo: float, hi: float) -> _abi.Prior:
        """0 on ``[lo, hi]``, -inf outside."""
        return _abi.Prior(_abi.CSSM_PRIOR_UNIFORM, 0, float(lo), float(hi))


def param_names(params: Parameters):
    """A name per slot of ``params.flattenParams()``: ``"<leaf>.scale"`` and ``"<leaf>.<field>[<i>]"`` (the SDE parameter's own field
    names, e.g. ``"0.phi[0]"``)."""
    import dataclasses
    names = []
    for l, node in enumerate(params.leaves):
        if node.scale is not None:
            names.append(f"{l}.scale")
        for fld in dataclasses.fields(node.sdeParam):
            names.extend(f"{l}.{fld.name}[{i}]" for i in range(len(getattr(node.sdeParam, fld.name))))
    return names


def priors_for(params: Parameters, priors) -> list:
    """The ``n_theta`` priors of ``pmmh_fleet_chains`` from a dict ``{slot index or name (param_names): Prior}``; every other slot is
    flat.  An unknown slot is refused."""
    names = param_names(params)
    out = [Prior.flat() for _ in names]
    for key, pr in dict(priors).items():
        if isinstance(key, str):
            if key not in names:
                raise ValueError(f"no parameter named {key!r} (the names are {names})")
            j = names.index(key)
        else:
            j = int(key)
            if not 0 <= j < len(names):
                raise ValueError(f"slot {j} outside the {len(names)} flattened parameters")
        if not isinstance(pr, _abi.Prior):
            raise ValueError(f"slot {key!r}: a Prior.flat() / .normal(mean, sd) / .uniform(lo, hi) is needed")
        out[j] = pr
    return out


def covariance(theta_rows) -> np.ndarray:
    """``Parameters.covariance(samples)`` (Parameters.scala:135-139): the sample covariance (denominator ``n - 1``) of flattened rows
    ``theta_rows[n, n_theta]`` -- a chain's ``theta`` output, or a sequence of Parameters."""
    rows = [np.asarray(r.flattenParams() if isinstance(r, Parameters) else r, dtype=np.float64) for r in theta_rows]
    m = np.atleast_2d(np.asarray(rows, dtype=np.float64))
    if m.shape[0] < 2:
        raise ValueError("the covariance of a sample needs two rows at least")
    return np.atleast_2d(np.cov(m, rowvar=False))


def perturbMvn(chol):
    """``Parameters.perturbMvn(chol)`` (Parameters.scala:111-114) as a proposal of the generic ``MetropolisHastings.pmmhState`` loop:
    ``p + chol z``, z standard normal, the innovations added in flatten order."""
    chol = np.atleast_2d(np.asarray(chol, dtype=np.float64))

    def proposal(p: Parameters, rng: np.random.Generator) -> Parameters:
        return p.add(chol @ rng.standard_normal(chol.shape[1]))
    return proposal


def perturbMvnEigen(eigvals, eigvecs):
    """``Parameters.perturbMvnEigen(eigen)`` (Parameters.scala:116-123): ``p + Q z`` with ``Q = eigvecs diag(sqrt(eigvals))`` -- the
    same innovation covariance as ``perturbMvn`` of the Cholesky factor."""
    q = np.asarray(eigvecs, dtype=np.float64) * np.sqrt(np.asarray(eigvals, dtype=np.float64))[None, :]

    def proposal(p: Parameters, rng: np.random.Generator) -> Parameters:
        return p.add(q @ rng.standard_normal(q.shape[1]))
    return proposal


def chol_from_pilot(theta_rows, scale: Optional[float] = None, jitter: float = 1e-12) -> np.ndarray:
    """The lower-triangular proposal factor of ``pmmh_fleet_chains`` from a pilot chain's rows ``theta_rows[n, n_theta]``:
    ``chol(scale * covariance + jitter I)`` over the slots that moved, zero rows (a fixed parameter) on those that did not.
    ``scale``: None = ``2.38**2 / n_free`` (Roberts, Gelman and Gilks 1997), n_free the slots that moved."""
    m = np.atleast_2d(np.asarray(theta_rows, dtype=np.float64))
    nt = m.shape[1]
    free = np.flatnonzero(m.max(axis=0) > m.min(axis=0))
    L = np.zeros((nt, nt))
    if free.size == 0:
        return L
    s = 2.38 ** 2 / free.size if scale is None else float(scale)
    cov = covariance(m[:, free]) * s + jitter * np.eye(free.size)
    L[np.ix_(free, free)] = np.linalg.cholesky(cov)
    return L


def pmmh_fleet_chains(unparam: UnparamModel, inits: Sequence[Parameters], datas, n: int, chol, priors=None, iters: int = 1000,
                      seeds: Optional[Sequence[int]] = None, first_iter: int = 0, ll0=None, state0=None, iters_per_launch: int = 0,
                      device: int = 0, fleet: Optional[NativePfFleet] = None):
    """``len(inits)`` whole chains on the device (``cssm_fleet_pmmh_chains``), a chain per series and every iteration of a chain inside
    one launch: the reference's PMMH with its ``prior`` argument (PMMH.scala:32,72-73) and its tuned proposal ``Parameters.perturbMvn``
    (Parameters.scala:111-114).  ``chol``: the proposal's lower-triangular factor ``[n_theta, n_theta]`` (``chol_from_pilot``; one per
    chain as ``[S, n_theta, n_theta]``); ``math.sqrt(delta) * np.eye(n_theta)`` with no priors is ``pmmh_native_fleet`` bit for bit.
    ``priors``: None, ``n_theta`` entries, or a dict for ``priors_for``.  ``first_iter`` / ``ll0`` / ``state0`` continue chains from their
    last rows.  Returns ``(ll[S, iters], theta[S, iters, n_theta], accepted[S, iters], last_state[S, iters, d], diag[S, 2])`` -- what
    ``pmmh_native_fleet`` returns, then per chain the proposals rejected unfiltered (outside the prior's support) and those whose filter
    had no usable weight; ``fleet_posterior_rows`` takes the first four as they are."""
    S = len(inits)
    if S < 1 or seeds is None or len(seeds) != S:
        raise ValueError("one seed per chain")
    theta0 = [np.asarray(p.flattenParams(), dtype=np.float64) for p in inits]
    if any(th.shape != theta0[0].shape for th in theta0):
        raise ValueError("every chain's initial parameters must flatten to the same length")
    theta0 = np.ascontiguousarray(theta0, dtype=np.float64)
    if isinstance(priors, dict):
        priors = priors_for(inits[0], priors)
    off, t, y, has = pmmh_fleet_pack(datas, S)
    model = unparam.run(inits[0])
    desc = model.descriptor()
    own = fleet is None
    if own:
        fleet = NativePfFleet(model, n, S, device)
    elif fleet.S != S or fleet.n != int(n):
        raise ValueError(f"the fleet holds {fleet.S} series of {fleet.n} particles, the run needs {S} of {n}")
    try:
        return fleet.pmmh_chains(desc, theta0, chol, off, t, y, has, seeds, iters, priors=priors, first_iter=first_iter, ll0=ll0,
                                 state0=state0, iters_per_launch=iters_per_launch)[:5]
    finally:
        if own:
            fleet.close()


LGCP_ITERS_PER_LAUNCH = 100   # the driver's default launch length for event streams (pmmh_lgcp_fleet_chains)


def pmmh_lgcp_fleet_chains(unparam: UnparamModel, inits: Sequence[Parameters], streams, n: int, precision: int, chol, priors=None,
                           iters: int = 1000, seeds: Optional[Sequence[int]] = None, first_iter: int = 0, ll0=None, state0=None,
                           iters_per_launch: Optional[int] = None, device: int = 0, fleet: Optional[NativeLgcpFleet] = None):
    """``pmmh_fleet_chains`` for log-Gaussian Cox processes (``cssm_fleet_pmmh_chains_lgcp``): ``len(inits)`` whole chains on the device
    over ``FilterLgcp(model, resample, precision)``, a chain per stream and every iteration and event of a chain inside one launch.
    ``unparam``: an LGCP model (``Model.lgcp``).  ``streams``: ONE array of event times (every chain sees it) or one per chain -- what
    ``NativeLgcpFleet.pack`` takes, e.g. ``simulate.lgcp_fleet_data``.  ``chol``, ``priors`` (None, ``n_theta`` entries, or a dict for
    ``priors_for``), ``first_iter`` / ``ll0`` / ``state0`` as ``pmmh_fleet_chains``; ``math.sqrt(delta) * np.eye(n_theta)`` with no priors
    is ``cssm_pmmh_run`` on an LGCP handle per chain, bit for bit.  ``iters_per_launch``: None = ``LGCP_ITERS_PER_LAUNCH`` (an event
    is a chain of sub-steps, so an iteration is heavy: at the recorded 3.54 ms per fleet filter of S = 1024, N = 1000 and 12 547 events
    that is about a third of a second per launch -- derived, not measured; a default, not a limit: 0 = all iterations in one launch);
    it never changes a bit.  ``fleet``: a NativeLgcpFleet of S streams, n particles and this precision to reuse.  Returns ``(ll[S,
    iters], theta[S, iters, n_theta], accepted[S, iters], last_state[S, iters, d], diag[S, 2])``; ``fleet_posterior_rows`` takes the
    first four as they are."""
    S = len(inits)
    if S < 1 or seeds is None or len(seeds) != S:
        raise ValueError("one seed per chain")
    theta0 = [np.asarray(p.flattenParams(), dtype=np.float64) for p in inits]
    if any(th.shape != theta0[0].shape for th in theta0):
        raise ValueError("every chain's initial parameters must flatten to the same length")
    theta0 = np.ascontiguousarray(theta0, dtype=np.float64)
    if isinstance(priors, dict):
        priors = priors_for(inits[0], priors)
    shared = len(streams) == 0 or np.ndim(streams[0]) == 0        # one array of times: every chain sees it
    streams = [streams] * S if shared else list(streams)
    if len(streams) != S:
        raise ValueError(f"one array of event times, or one per chain ({S}), not {len(streams)}")
    off, t, _, _ = NativeLgcpFleet.pack(streams)                  # (refuses a stream without events, before any device call)
    model = unparam.run(inits[0])
    desc = model.descriptor(int(precision))
    per = LGCP_ITERS_PER_LAUNCH if iters_per_launch is None else int(iters_per_launch)
    own = fleet is None
    if own:
        fleet = NativeLgcpFleet(model, n, S, int(precision), device)
    elif fleet.S != S or fleet.n != int(n) or getattr(fleet, "precision", None) != int(precision):
        raise ValueError(f"the fleet holds {fleet.S} streams of {fleet.n} particles at precision {getattr(fleet, 'precision', None)}, "
                         f"the run needs {S} of {n} at {int(precision)}")
    try:
        return fleet.pmmh_chains_lgcp(desc, theta0, chol, off, t, seeds, iters, priors=priors, first_iter=first_iter, ll0=ll0,
                                      state0=state0, iters_per_launch=per)[:5]
    finally:
        if own:
            fleet.close()


def pmmh_native_speculative(unparam: UnparamModel, init: Parameters, data, n: int, delta: float, iters: int,
                            seed: int = 20260101, device: int = 0):
    """``pmmh_native`` -- the same chain, bit for bit -- at two iterations per batch of three filters (``cssm_pmmh_run_speculative``):
    iteration i's proposal and both candidates for iteration i + 1 (proposed from it, and from the current parameters) are filtered
    together; the proposals and filter keys are functions of (seed, iteration, parameters) alone.  For clouds that leave the GPU
    mostly idle (BASELINE configs[4]: N = 100 000).  Returns (ll[iters], theta[iters, n_theta], accepted[iters], last_state[iters, d])."""
    t, y, h = split_data(data)
    model = unparam.run(init)
    desc = model.descriptor()
    lib = _abi.load_library()
    hb = C.c_void_p()
    _abi.check(lib.cssm_pfb_create(desc.ptr(), int(n), 3, int(device), C.byref(hb)))
    try:
        d = int(lib.cssm_pf_dim(lib.cssm_pfb_chain(hb, 0)))
        theta0 = np.ascontiguousarray(init.flattenParams(), dtype=np.float64)
        nt = theta0.size
        ll = np.zeros(iters); th = np.zeros((iters, nt)); acc = np.zeros(iters, dtype=np.int32); last = np.zeros((iters, d))
        dp = C.POINTER(C.c_double)
        _abi.check(lib.cssm_pmmh_run_speculative(hb, desc.ptr(), theta0.ctypes.data_as(dp), nt, float(delta), t.ctypes.data_as(dp), y.ctypes.data_as(dp),
                                                 h.ctypes.data_as(C.POINTER(C.c_uint8)), len(t), int(seed) & (2**64 - 1), int(iters),
                                                 ll.ctypes.data_as(dp), th.ctypes.data_as(dp), acc.ctypes.data_as(C.POINTER(C.c_int32)), last.ctypes.data_as(dp)))
    finally:
        lib.cssm_pfb_destroy(hb)
    return ll, th, acc, last


def posterior_rows(theta, last_state, burn_in: int = 0, thin: int = 1):
    """The posterior sample of a chain's output arrays (theta[iters, n_theta], last_state[iters, d]): the rows formats.read_pmmh_json
    keeps of the same chain written one MetropState per line -- ``burn_in`` dropped, then every ``thin``-th."""
    if burn_in < 0 or thin < 1:
        raise ValueError("burn_in >= 0 and thin >= 1")
    theta = np.atleast_2d(np.asarray(theta, dtype=np.float64))
    last_state = np.asarray(last_state, dtype=np.float64).reshape(theta.shape[0], -1)
    keep = np.arange(burn_in, theta.shape[0], thin)
    return theta[keep], last_state[keep]


def fleet_posterior_rows(theta, last_state, burn_in: int = 0, thin: int = 1):
    """``posterior_rows`` of every chain of ``pmmh_native_fleet``'s output (theta[S, iters, n_theta], last_state[S, iters, d]): a list of
    S ``(theta_k, last_state_k)`` pairs, what ``NativePfFleet.forecast_posterior`` and ``FilterFleet.forecastPosterior`` (with
    ``params``) take as their posteriors."""
    theta = np.asarray(theta, dtype=np.float64)
    last_state = np.asarray(last_state, dtype=np.float64)
    if theta.ndim != 3 or last_state.ndim != 3 or last_state.shape[:2] != theta.shape[:2]:
        raise ValueError("theta[S, iters, n_theta] and last_state[S, iters, d] of pmmh_native_fleet")
    return [posterior_rows(theta[k], last_state[k], burn_in, thin) for k in range(theta.shape[0])]
