#!/usr/bin/env python3
"""simulate_lgcp_probe.py -- SimulateData.simLGCP on the device (cssm_simulate_lgcp: k_lgcp_grid, one thread per pair of paths over the
whole grid; k_lgcp_thin, one thread per path, run twice: count, then write).  One JSON line per shape.

Shape: model C4 (Model.lgcp(Sde.ouProcess(1)), ouParameter(0.1)(0.5)(0.4)(0.1)(0.5)) on [0, 10] at precision 2 (1001 grid points),
n_paths = 1, 1024 and 65 536, the grid rows not kept (the events carry their states).  Measured per call: wall time around
cssm_simulate_lgcp and the reading of its result object (plan, uploads, the launches of every chunk, the read-back of counts and events),
and the device time of its kernels (cssm_simulate_lgcp_last_ms: HIP events around the grid kernels / the thinning launches) -- each the
median of --repeats calls after --warmup calls of the same shape, with the smallest and the largest beside it, Python's collector off.

Baseline.  The parent of this feature has no counterpart: nothing drew event times from the model.  What stands beside the figures is
the host twin of the thinning statements (tests/cpp/lgcp_thin_twin.c, gcc -O2) looped over the paths on ONE core, fed the device's own
eta columns (at most --twin-paths paths timed, --spread times, scaled linearly to n_paths: exact for a sequential loop).  It covers the
thinning only, not the grid; it is a baseline to read the thinning launches against, not a competing implementation.

Kernel times of their own come from a run under `rocprofv3 --kernel-trace --stats -- python tools/simulate_lgcp_probe.py ...`."""
from __future__ import annotations

import argparse
import gc
import json
import math
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import cases  # noqa: E402
from composablestatespacemodels_amd.simulate import sim_key, simulate_lgcp, simulate_lgcp_last_ms  # noqa: E402
from fleet_probe import timed  # noqa: E402
from test_simulate_lgcp_host import build_lgcp_twin, twin_thin  # noqa: E402


def spread(v):
    return [round(min(v), 4), round(max(v), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", default="1,1024,65536")
    ap.add_argument("--start", type=float, default=0.0)
    ap.add_argument("--end", type=float, default=10.0)
    ap.add_argument("--precision", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--twin-paths", type=int, default=1024, help="paths the host twin's loop is timed on (scaled to n_paths)")
    ap.add_argument("--spread", type=int, default=3, help="repeats of the host twin's loop")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    model = cases.c4_model()
    key = sim_key(cases.SEED)
    delta = math.pow(10, -a.precision)
    lines = []
    twin = None if a.no_baseline else build_lgcp_twin(tempfile.mkdtemp(prefix="lgcp_twin_"))
    gc.disable()
    for n in [int(x) for x in a.paths.split(",")]:
        def call():
            s = simulate_lgcp(model, a.start, a.end, a.precision, n, key, keep_grid=False)
            return simulate_lgcp_last_ms() + (len(s.ev_t), int(s.candidates.sum()), int((s.status != 0).sum()))
        r = timed(call, a.repeats, a.warmup)
        wall = [w * 1e3 for w, _ in r]
        grid_ms, thin_ms = [e[0] for _, e in r], [e[1] for _, e in r]
        line = {"probe": "simulate_lgcp", "model": "c4", "interval": [a.start, a.end], "precision": a.precision, "n_paths": n, "repeats": a.repeats,
                "events": r[0][1][2], "candidates": r[0][1][3], "flagged_paths": r[0][1][4],
                "wall_ms": round(statistics.median(wall), 4), "wall_min_max_ms": spread(wall),
                "k_lgcp_grid_ms": round(statistics.median(grid_ms), 4), "k_lgcp_grid_min_max_ms": spread(grid_ms),
                "k_lgcp_thin_ms": round(statistics.median(thin_ms), 4), "k_lgcp_thin_min_max_ms": spread(thin_ms)}
        if twin is not None:
            m = min(n, a.twin_paths)
            s = simulate_lgcp(model, a.start, a.end, a.precision, m, key, keep_grid=True)
            d = s.grid.shape[1] - 3
            eta = [np.ascontiguousarray(s.grid[:, d + 1, i]) for i in range(m)]

            def loop():
                return sum(len(twin_thin(twin, key, i, s.grid_t, eta[i], a.start, a.end, delta, float(s.upper[i]))[1]) for i in range(m))
            tl = timed(loop, a.spread, 1)
            assert tl[0][1] == int(s.ev_off[m])                      # the same events
            ms = [w * 1e3 for w, _ in tl]
            line.update({"twin_paths": m, "twin_loop_ms": round(statistics.median(ms), 4), "twin_loop_min_max_ms": spread(ms),
                         "twin_loop_scaled_ms": round(statistics.median(ms) * n / m, 4)})
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
