#!/usr/bin/env python3
"""fleet_pmmh_chains_probe.py -- whole PMMH chains on the device (cssm_fleet_pmmh_chains, k_fleet_pmmh) against cssm_fleet_pmmh_run (a
launch, S model builds, S x T record builds, an upload and a read-back per iteration) on the same build and the same fleet.  One JSON
line per N.

Shape: model C2 (d = 3, 10 stored parameters), S = 1024 chains over T = 100 records, 20 iterations, flat priors and the diagonal factor
sqrt(delta) I -- the two calls then compute the same chains bit for bit (asserted on every repeat).  Measured: wall time around each call
and, for the new call, the device time of its launches (cssm_fleet_pmmh_chains_last_ms); for the old one its own split
(cssm_fleet_pmmh_last_split: propose + set_params + reseed | record building | upload | kernel | decisions, summed over the iterations).
The two calls alternate, --repeats of each after --warmup of each; medians with minimum and maximum, Python's collector off.

Derived: old wall / new wall, and nanoseconds of device time per (chain, iteration, record, particle) next to k_fleet_if2's."""
from __future__ import annotations

import argparse
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
from composablestatespacemodels_amd.filter import NativePfFleet  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="100,1000,4096")
    ap.add_argument("--series", type=int, default=1024)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--delta", type=float, default=0.02)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    model = cases.c2_model()
    th = np.array(model.parameters().flattenParams())
    S, T, M = a.series, a.T, a.iters
    seven = [cases.poisson_counts(T, seed=cases.SEED + k, missing=0.1) for k in range(7)]              # (seven distinct series, repeated)
    packed = NativePfFleet.pack([seven[k % 7] for k in range(S)])
    theta0 = np.ascontiguousarray([th + 0.01 * ((k % 5) - 2) for k in range(S)])
    seeds = [cases.SEED + k for k in range(S)]
    L = math.sqrt(a.delta) * np.eye(len(th))
    lines = []
    gc.disable()
    for n in (int(x) for x in a.n.split(",")):
        with NativePfFleet(model, n, S) as fl:
            desc = model.descriptor()
            old_w, new_w, new_d, splits = [], [], [], []
            for r in range(a.warmup + a.repeats):
                t0 = time.perf_counter()
                want = fl.pmmh_run(desc, theta0, a.delta, *packed, seeds, M)
                t1 = time.perf_counter()
                got = fl.pmmh_chains(desc, theta0, L, *packed, seeds, M)
                t2 = time.perf_counter()
                for u, v in zip(got[:4], want):
                    assert np.array_equal(u, v), "the two calls differ"
                if r >= a.warmup:
                    old_w.append(t1 - t0); new_w.append(t2 - t1); new_d.append(fl.pmmh_chains_last_ms()); splits.append(fl.pmmh_last_split()[0])
        med = statistics.median
        steps = float(S) * M * T * n
        line = {"probe": "fleet_pmmh_chains", "model": "c2", "d": 3, "n_theta": len(th), "n": n, "S": S, "T": T, "iters": M, "repeats": a.repeats,
                "old_wall_ms": round(med(old_w) * 1e3, 3), "old_wall_min_ms": round(min(old_w) * 1e3, 3), "old_wall_max_ms": round(max(old_w) * 1e3, 3),
                "old_split_ms": [round(med(s[q] for s in splits), 3) for q in range(5)],
                "new_wall_ms": round(med(new_w) * 1e3, 3), "new_wall_min_ms": round(min(new_w) * 1e3, 3), "new_wall_max_ms": round(max(new_w) * 1e3, 3),
                "new_device_ms": round(med(new_d), 3), "new_device_min_ms": round(min(new_d), 3), "new_device_max_ms": round(max(new_d), 3),
                "old_over_new_wall": round(med(old_w) / med(new_w), 2),
                "old_kernel_over_new_device": round(med(s[3] for s in splits) / med(new_d), 3),
                "ns_per_particle_step": round(med(new_d) * 1e-3 / steps * 1e9, 4)}
        print(json.dumps(line), flush=True)
        lines.append(line)
    gc.enable()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
