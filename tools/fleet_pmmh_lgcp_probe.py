#!/usr/bin/env python3
"""fleet_pmmh_lgcp_probe.py -- whole PMMH chains for LGCP fleets on the device (cssm_fleet_pmmh_chains_lgcp, k_fleet_pmmh_lgcp) against
the route the library offered before on the same LGCP fleet and build: a host loop of set_params + reseed + filter per iteration
(cssm_fleet_set_params, _reseed, _filter: S model builds, S x T record builds, an upload, a launch and a read-back per iteration), with
the proposals and decisions of cssm_pmmh_run formed on the host from the contract's streams.  One JSON line per N.

Shape: model C4 (d = 1, 5 stored parameters) at precision 2, event streams from simulate_lgcp on [0, 10], S = 1024 chains, 20
iterations, flat priors and L = sqrt(0.02) I -- the two routes then compute the same chains bit for bit (asserted on every repeat).
Measured: wall time around each route; the device time of the new call's launches (cssm_fleet_pmmh_chains_lgcp_last_ms); the host
loop's split (propose | set_params | reseed | filter wall, of which device | decide, summed over the iterations).  The two routes
alternate, --repeats of each after --warmup of each; medians with minimum and maximum, Python's collector off.

Derived: old wall / new wall, and nanoseconds of device time per (chain, iteration, particle, sub-step) of both routes, next to the
LGCP fleet filter's recorded figure (profiles/fleet_lgcp_probe.jsonl)."""
from __future__ import annotations

import argparse
import ctypes as C
import gc
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cases  # noqa: E402
import pmmh_chain_twin as twin  # noqa: E402
from composablestatespacemodels_amd import _abi  # noqa: E402
from composablestatespacemodels_amd.filter import NativeLgcpFleet  # noqa: E402
from composablestatespacemodels_amd.model import UnparamModel  # noqa: E402
from composablestatespacemodels_amd.simulate import lgcp_fleet_data, simulate_lgcp  # noqa: E402
from oracle import oracle  # noqa: E402

PRECISION = 2


def sub_steps(lib, desc, t):
    """the sub-steps of one stream as the records hold them (cssm_fleet_pmmh_lgcp_pack_record)"""
    buf, nb, nf = (C.c_uint8 * 256)(), C.c_size_t(), C.c_size_t()
    total, tp = 0, float(np.min(t))
    for s, tt in enumerate(t):
        _abi.check(lib.cssm_fleet_pmmh_lgcp_pack_record(desc.ptr(), tp, float(tt), s, buf, 256, C.byref(nb), None, 0, C.byref(nf)))
        total += int(np.frombuffer(bytes(buf[8:12]), dtype=np.int32)[0])
        tp = float(tt)
    return total


def host_loop(fl, um, p0, theta0, sd, packed, seeds, iters, split):
    """cssm_pmmh_run of every chain as a host loop over the fleet's own calls: (ll, theta, accepted, last_state), chain-major"""
    S, nt = theta0.shape
    cur, cur_ll, cur_st, acc = theta0.copy(), np.full(S, -1e99), np.zeros((S, fl.d)), np.zeros(S, dtype=np.int32)
    out = (np.zeros((S, iters)), np.zeros((S, iters, nt)), np.zeros((S, iters), dtype=np.int32), np.zeros((S, iters, fl.d)))
    for it in range(iters):
        t0 = time.perf_counter()
        z = np.array([twin.proposal_normals(seeds[k], it, nt) for k in range(S)])
        prop = cur + sd * z
        keys = [twin.filter_key(seeds[k], it) for k in range(S)]
        t1 = time.perf_counter()
        fl.set_params([um.run(p0.withFlat(prop[k])) for k in range(S)])
        t2 = time.perf_counter()
        fl.reseed(keys)
        t3 = time.perf_counter()
        ll, _, _, _, last, rc = fl.filter_packed(*packed, want_path=False)
        t4 = time.perf_counter()
        dev = fl.last_ms()[0]
        ll = np.where(rc == _abi.CSSM_ENONFINITE, -np.inf, ll)
        logu = oracle.c_log([twin.accept_uniform(seeds[k], it) for k in range(S)])
        take = np.asarray(logu) < (ll - cur_ll)
        cur[take], cur_ll[take], cur_st[take] = prop[take], ll[take], last[take]
        acc += take
        out[0][:, it], out[1][:, it], out[2][:, it], out[3][:, it] = cur_ll, cur, acc, cur_st
        t5 = time.perf_counter()
        for j, v in enumerate((t1 - t0, t2 - t1, t3 - t2, t4 - t3, dev / 1e3, t5 - t4)):
            split[j] += v * 1e3
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="100,1000,4096")
    ap.add_argument("--series", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--delta", type=float, default=0.02)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    model = cases.c4_model()
    um, p0 = UnparamModel([l[0] for l in model.leaves]), model.parameters()
    th = np.array(p0.flattenParams())
    S, M = a.series, a.iters
    sim = simulate_lgcp(model, 0.0, 10.0, PRECISION, n_paths=64, keep_grid=False)
    distinct = [s for s in lgcp_fleet_data(sim) if len(s) > 0]
    streams = [distinct[k % len(distinct)] for k in range(S)]
    packed = NativeLgcpFleet.pack(streams)
    theta0 = np.ascontiguousarray([th + 0.01 * ((k % 5) - 2) for k in range(S)])
    seeds = [cases.SEED + k for k in range(S)]
    sd = math.sqrt(a.delta)
    L = sd * np.eye(len(th))
    desc = model.descriptor(PRECISION)
    lib = _abi.load_library()
    per_stream = [sub_steps(lib, desc, s) for s in distinct]
    subs = sum(per_stream[k % len(distinct)] for k in range(S))
    events = int(packed[0][-1])
    lines = []
    gc.disable()
    for n in (int(x) for x in a.n.split(",")):
        with NativeLgcpFleet(model, n, S, PRECISION) as fl:
            old_w, new_w, new_d, splits = [], [], [], []
            for r in range(a.warmup + a.repeats):
                split = [0.0] * 6
                t0 = time.perf_counter()
                want = host_loop(fl, um, p0, theta0, sd, packed, seeds, M, split)
                t1 = time.perf_counter()
                got = fl.pmmh_chains_lgcp(desc, theta0, L, packed[0], packed[1], seeds, M)
                t2 = time.perf_counter()
                assert not got[5].any() and not got[4].any()
                for x, y in zip(got[:4], want):
                    assert np.array_equal(x, y), "the two routes differ"
                if r >= a.warmup:
                    old_w.append(t1 - t0); new_w.append(t2 - t1); new_d.append(fl.pmmh_chains_lgcp_last_ms()); splits.append(split)
            mmm = lambda v, s=1.0: [round(statistics.median(v) * s, 3), round(min(v) * s, 3), round(max(v) * s, 3)]
            sp = [round(statistics.median([q[j] for q in splits]), 3) for j in range(6)]
            per = 1e6 / (float(M) * n * subs)
            line = {"probe": "fleet_pmmh_lgcp", "model": "c4", "d": 1, "n_theta": len(th), "precision": PRECISION, "n": n, "S": S, "events": events,
                    "sub_steps": subs, "iters": M, "repeats": a.repeats, "warmup": a.warmup,
                    "host_loop_wall_ms": mmm(old_w, 1e3),
                    "host_loop_split_ms": dict(zip(("propose", "set_params", "reseed", "filter_wall", "filter_device", "decide"), sp)),
                    "chains_lgcp_wall_ms": mmm(new_w, 1e3), "chains_lgcp_device_ms": mmm(new_d),
                    "old_over_new_wall": round(statistics.median(old_w) / statistics.median(new_w), 2),
                    "ns_per_chain_iter_particle_substep": {"chains_lgcp_device": round(statistics.median(new_d) * per, 5),
                                                           "host_loop_filter_device": round(sp[4] * per, 5)},
                    "accepted_of_iters_mean": round(float(got[2][:, -1].mean()), 2)}
            print(json.dumps(line), flush=True)
            lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
