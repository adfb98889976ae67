"""The sequential host twin of ``cssm_fleet_pmmh_chains``: one chain, written from include/cssm_numerics.h ("PMMH chains on the device")
over what the oracle exports -- the proposal's normals (``oracle.c_normals``, tag 4 = CSSM_STREAM_HOST), the acceptance uniform, the
contract's log, the key derivation -- and, for the filter, ``OraclePf.set_params`` / ``reseed`` / ``filter(want_path=True)``.  Every
product and sum is an IEEE double operation of its own (Python floats), in the header's order.  ``ll_fn`` replaces the particle filter
(e.g. by an exact likelihood): ``ll_fn(theta, key) -> (ll, last_state)``; a filter without a usable weight returns ``(-inf, None)``."""
import math

import numpy as np

from composablestatespacemodels_amd import _abi
from oracle import oracle

STREAM_HOST = 4
NEG_INF = float("-inf")


def prior_term(kind, a, b, theta):
    """cssm_prior_term"""
    if kind == _abi.CSSM_PRIOR_NORMAL:
        z = (theta - a) / b
        return -(z * z) / 2.0
    if kind == _abi.CSSM_PRIOR_UNIFORM:
        return 0.0 if (a <= theta <= b) else NEG_INF
    return 0.0


def log_prior(priors, theta):
    """lp(theta): 0.0, then the non-flat terms added left to right"""
    lp = 0.0
    if priors is None:
        return lp
    for pr, th in zip(priors, theta):
        if pr.kind != _abi.CSSM_PRIOR_FLAT:
            lp = lp + prior_term(pr.kind, pr.a, pr.b, float(th))
    return lp


def proposal_normals(seed, it, nt):
    """z_j = element j & 1 of cssm_normal_pair_of(seed, it, j >> 1, CSSM_STREAM_HOST, 0)"""
    z = []
    for pair in range((nt + 1) // 2):
        z.extend(float(v) for v in oracle.c_normals(seed, it, pair, STREAM_HOST, 0, 1)[0])
    return z[:nt]


def propose(L, z, cur):
    """cssm_chain_propose per slot"""
    out = []
    for i, c in enumerate(cur):
        s, any_ = 0.0, False
        for j in range(i + 1):
            lij = float(L[i][j])
            if lij != 0.0:
                p = lij * z[j]
                s = s + p if any_ else p
                any_ = True
        out.append(float(c) + s if any_ else float(c))
    return out


def accept_uniform(seed, it):
    return float(oracle.lib().oracle_c_mh_u(seed, it))


def filter_key(seed, it):
    return int(oracle.lib().oracle_c_derive_key(seed, it + 1))


def oracle_ll_fn(unparam, params0, n, t, y, has):
    """The default ``ll_fn``: the oracle's ``filter`` under the proposal and the key -- (ll, row T of its sampled path); a filter without
    a usable weight is (-inf, None)."""
    state = {"pf": None}

    def ll_fn(theta, key):
        desc = unparam.run(params0.withFlat(theta)).descriptor()
        if state["pf"] is None:
            state["pf"] = oracle.OraclePf(desc, n, key)
        else:
            state["pf"].set_params(desc)
        state["pf"].reseed(key)
        try:
            ll, _, _, path = state["pf"].filter(t, y, has, want_path=True)
        except oracle.OracleError as e:
            if e.code != _abi.CSSM_ENONFINITE:
                raise
            return NEG_INF, None
        return float(ll), np.array(path[-1])
    return ll_fn


def run_chain(ll_fn, theta0, L, priors, seed, n_iters, d, first_iter=0, ll0=None, state0=None, accept_all=False):
    """One chain of ``n_iters`` iterations.  Returns ``(ll[n_iters], theta[n_iters, nt], accepted[n_iters], last_state[n_iters, d],
    diag[2])``.  ``accept_all``: every filtered proposal is accepted (a random walk: what a broken decision would do -- for the tests
    that must be able to tell)."""
    cur = [float(v) for v in theta0]
    nt = len(cur)
    cur_ll = -1e99 if ll0 is None else float(ll0)
    cur_state = np.zeros(d) if state0 is None else np.array(state0, dtype=np.float64)
    lp_cur = log_prior(priors, cur)
    if not lp_cur > NEG_INF:
        raise ValueError("theta0 lies outside the prior's support")
    acc, diag = 0, [0, 0]
    out_ll, out_th, out_acc, out_st = np.zeros(n_iters), np.zeros((n_iters, nt)), np.zeros(n_iters, dtype=np.int32), np.zeros((n_iters, d))
    for q in range(n_iters):
        it = first_iter + q
        prop = propose(L, proposal_normals(seed, it, nt), cur)
        lp_prop = log_prior(priors, prop)
        u = accept_uniform(seed, it)
        if not lp_prop > NEG_INF:
            diag[0] += 1
        else:
            ll_prop, st = ll_fn(prop, filter_key(seed, it))
            if st is None:
                ll_prop = NEG_INF
                diag[1] += 1
            a = ((ll_prop + lp_prop) - cur_ll) - lp_cur
            if (accept_all and st is not None) or float(oracle.c_log([u])[0]) < a:
                cur, cur_ll, lp_cur, cur_state = prop, ll_prop, lp_prop, np.array(st, dtype=np.float64)
                acc += 1
        out_ll[q], out_th[q], out_acc[q], out_st[q] = cur_ll, cur, acc, cur_state
    return out_ll, out_th, out_acc, out_st, np.array(diag, dtype=np.uint32)
