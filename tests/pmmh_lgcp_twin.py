"""The LGCP side of the sequential twin of whole PMMH chains (tests/pmmh_chain_twin.py): an ``ll_fn`` for ``run_chain`` over the oracle's
FilterLgcp -- the filter of include/cssm_numerics.h, "PMMH chains on the device: LGCP" --, and the event streams and proposal cases the
host and the device tests of ``cssm_fleet_pmmh_chains_lgcp`` share.  ``run_chain`` itself is the plain twin's, unchanged."""
import numpy as np

import cases
from composablestatespacemodels_amd import _abi
from composablestatespacemodels_amd.model import UnparamModel
from composablestatespacemodels_amd.pmmh import Prior
from oracle import oracle
from pmmh_chain_twin import NEG_INF, run_chain  # noqa: F401  (run_chain: what the callers of this module drive)

SEED = cases.SEED
PRECISION = 2
MODELS = {"c4": cases.c4_model, "seasonal": cases.lgcp_seasonal_model}


def unparam_of(model):
    return UnparamModel([l[0] for l in model.leaves])


def events(t):
    t = np.ascontiguousarray(t, dtype=np.float64)
    return t, np.ones(len(t)), np.ones(len(t), dtype=np.uint8)


def stream(T, seed, repeat=None):
    """T event times sorted on [0, 3], rounded to 3 decimals; ``repeat``: event ``repeat + 1`` takes the time of event ``repeat`` (an
    event with n_sub == 0 in mid-stream)"""
    t = cases.event_times(T, seed=seed, horizon=3.0)[0].copy()
    if repeat is not None:
        t[repeat + 1] = t[repeat]
    assert np.all(np.diff(t) >= 0.0)
    return t


def stream30():
    return stream(30, SEED + 3, repeat=11)


def lgcp_ll_fn(unparam, params0, n, t, precision=PRECISION):
    """``ll_fn(theta, key) -> (ll, last_state)`` of ``run_chain``: the oracle's FilterLgcp over the events ``t`` under the proposal and
    the key -- its ll and row T of its sampled path; a filter without a usable weight is (-inf, None)."""
    state = {"pf": None}
    ev = events(t)

    def ll_fn(theta, key):
        desc = unparam.run(params0.withFlat(theta)).descriptor(precision)
        if state["pf"] is None:
            state["pf"] = oracle.OraclePf(desc, n, key)
        else:
            state["pf"].set_params(desc)
        state["pf"].reseed(key)
        try:
            ll, _, _, path = state["pf"].filter(*ev, want_path=True)
        except oracle.OracleError as e:
            if e.code != _abi.CSSM_ENONFINITE:
                raise
            return NEG_INF, None
        return float(ll), np.array(path[-1])
    return ll_fn


def dense_case(name):
    """(model, L, priors): a dense lower-triangular factor with a zero row and an inner zero, a NORMAL prior and a UNIFORM prior whose
    bound lies +- 0.25 around the start"""
    model = MODELS[name]()
    th = np.array(model.parameters().flattenParams())
    nt = len(th)
    rng = np.random.default_rng(SEED + 9 + nt)
    L = np.tril(rng.uniform(-0.1, 0.1, size=(nt, nt))) + 0.25 * np.eye(nt)
    L[1, :] = 0.0                                                 # slot 1 stays fixed
    L[3, 1] = 0.0                                                 # a zero inside a row is skipped
    priors = [Prior.flat()] * nt
    priors[2] = Prior.normal(th[2] + 0.1, 0.5)
    priors[4] = Prior.uniform(th[4] - 0.25, th[4] + 0.25)
    return model, L, priors
