#!/usr/bin/env python3
"""fleet_if2_probe.py -- iterated filtering on a fleet (cssm_fleet_if2, an EXTENSION: maximum likelihood by IF2, S searches in one
launch) measured.  One JSON line per shape; the protocol of fleet_smooth_probe.py.  There is no parent counterpart: the project had no
likelihood maximiser, so nothing is gated on a ratio.

Shape: model C2 (d = 3, 10 stored parameters, the six that are not m0 / c0 random-walk before every record), S = 1024 searches of
N = 1000 particles over T = 100 records, M = 50 iterations.  Measured: wall time around the call -- the S x T records built on the host,
the upload of the starting swarm and the read-back included; it ends in the stream's synchronise -- and the device time of its launches
(cssm_fleet_if2_last_ms), median of --repeats calls after --warmup calls of the same shape with their minimum and maximum, Python's
collector off.

Derived: nanoseconds of device time per (search, iteration, record, particle) -- S x M x T x N particle steps, each the gather and
perturbation of a parameter row, d coefficient sets, d transitions, a density and its share of the resampling.

Against: the sequential twin (tests/cpp/if2_twin.c) on one host core over one search of --twin-M iterations, as a baseline only."""
from __future__ import annotations

import argparse
import gc
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import cases  # noqa: E402
from composablestatespacemodels_amd.filter import NativePfFleet  # noqa: E402
from fleet_probe import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="1000")
    ap.add_argument("--series", default="1024")
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--per-launch", type=int, default=0, help="iterations per launch (0: all in one)")
    ap.add_argument("--rw-sd", type=float, default=0.02)
    ap.add_argument("--cooling", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--twin-M", type=int, default=2, help="iterations of the host twin's search; 0: no twin")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    model = cases.c2_model()
    th = np.array(model.parameters().flattenParams())
    sd = np.full(len(th), a.rw_sd)
    T, M = a.T, a.iters
    lines = []
    gc.disable()
    for n in (int(x) for x in a.n.split(",")):
        for S in (int(x) for x in a.series.split(",")):
            seven = [cases.poisson_counts(T, seed=cases.SEED + k, missing=0.1) for k in range(7)]      # (seven distinct series, repeated)
            datas = [seven[k % 7] for k in range(S)]
            theta0 = np.array([th + 0.05 * ((k % 5) - 2) for k in range(S)])
            seeds = [cases.SEED + k for k in range(S)]
            with NativePfFleet(model, n, S) as fl:
                def search():
                    out = fl.if2(model.descriptor(), datas, sd, a.cooling, M, seeds, theta0=theta0, iters_per_launch=a.per_launch)
                    assert not out["rc"].any()
                    return fl.if2_last_ms()
                rs = timed(search, a.repeats, a.warmup)
            wall, dev = statistics.median(w for w, _ in rs), statistics.median(m for _, m in rs)
            steps = float(S) * M * T * n
            line = {"probe": "fleet_if2", "model": "c2", "d": 3, "n_theta": len(th), "n": n, "S": S, "T": T, "iters": M,
                    "iters_per_launch": a.per_launch, "repeats": a.repeats, "wall_ms": round(wall * 1e3, 3),
                    "wall_min_ms": round(min(w for w, _ in rs) * 1e3, 3), "wall_max_ms": round(max(w for w, _ in rs) * 1e3, 3),
                    "device_ms": round(dev, 3), "device_min_ms": round(min(m for _, m in rs), 3), "device_max_ms": round(max(m for _, m in rs), 3),
                    "ns_per_particle_step": round(dev * 1e-3 / steps * 1e9, 4)}
            if a.twin_M > 0:
                from test_fleet_if2_host import twin_search
                t0 = time.perf_counter()
                twin_search(model, n, datas[0], sd, a.cooling, a.twin_M, seeds[0], theta0=theta0[0])
                line["twin_one_core_ns"] = round((time.perf_counter() - t0) / (a.twin_M * T * n) * 1e9, 1)
                line["twin_over_device"] = round(line["twin_one_core_ns"] / line["ns_per_particle_step"], 1)
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
