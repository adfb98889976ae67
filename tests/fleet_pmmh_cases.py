"""Shared by test_fleet_pmmh_host.py and test_gpu_fleet_pmmh.py: the six PMMH chains of the fleet tests and their oracle runs, computed
once per process.  Chain k: model C2 started at test_gpu_fleet's ``_perturbed`` parameters, on data, missing pattern and seed of its own."""
import functools

import numpy as np

import cases
from oracle import oracle
from test_gpu_fleet import _perturbed

SEED = cases.SEED
CHAINS, ITERS = 6, 40


def chain_inits():
    return [_perturbed(cases.c2_params, k) for k in range(CHAINS)]


def chain_arrays(k):
    return cases.poisson_counts(12 + 3 * k, seed=SEED + k, missing=(0, .15, .4)[k % 3])


def chain_data(k):
    from composablestatespacemodels_amd import Data
    return [Data(float(a), float(b) if h else None) for a, b, h in zip(*chain_arrays(k))]


def chain_seed(k):
    return SEED + 100 + k


@functools.lru_cache(maxsize=None)
def oracle_chain(k, n, delta, iters=ITERS):
    """(ll, theta, accepted, last) of chain k from the oracle's pmmh; read-only arrays"""
    model = cases.c2_unparam().run(chain_inits()[k])
    o = oracle.OraclePf(model.descriptor(), n, 1)
    out = o.pmmh(model.descriptor(), np.array(chain_inits()[k].flattenParams()), delta, *chain_arrays(k), seed=chain_seed(k), n_iters=iters)
    for a in out:
        a.setflags(write=False)
    return out
