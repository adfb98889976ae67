#!/usr/bin/env python3
"""simulate_probe.py -- SimulateData on the device (cssm_simulate: k_simulate; cssm_fleet_simulate: k_fleet_simulate, one thread per
(series, pair of paths)) against what a user had before it, in the same process on the same GPU.  One JSON line per shape.

Fleet shape: model C2 (d = 3), S series of T times each, n_paths paths per series.  Measured: wall time around cssm_fleet_simulate (the
records of every series built on the host, one upload, one launch per chunk, the read-back; it ends in the stream's synchronise) and
the call's device time (cssm_fleet_simulate_last_ms: HIP events around upload, launches and read-back), median of --repeats calls after
warm-up calls of the same shape, Python's collector off; the ragged arrays are packed once outside the timed window.
Against: the same rows by a loop of cssm_simulate calls, one per series, through the C ABI with descriptors and output arrays made
beforehand (which favours the loop).  64 series timed, --spread times, scaled linearly to S (exact for a sequential loop); the spread
of those repeats is the margin the fleet figure has to clear.

Single shape: cssm_simulate of n_paths paths over T times -- wall time, and the device time of its kernels (cssm_simulate_last_ms: HIP
events around every k_simulate launch, summed over the chunks).  Against: cssm_pf_forecast with samples over the same T times from a
handle of n_paths particles just initialised -- the device time of its k_forecast launches (cssm_pf_forecast_last_ms()[0]; its selection
and finishing kernels, [1], are reported beside it).  k_simulate runs one time index more (the row at t0) and does strictly less per
index: no order keys, no partial sums, no barriers.

Kernel times of their own come from a run under `rocprofv3 --kernel-trace --stats -- python tools/simulate_probe.py ...`."""
from __future__ import annotations

import argparse
import ctypes as C
import gc
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import cases  # noqa: E402
from composablestatespacemodels_amd import _abi  # noqa: E402
from composablestatespacemodels_amd.filter import FilterFleet, NativePf, NativePfFleet  # noqa: E402
from composablestatespacemodels_amd.simulate import fleet_keys, sim_key, simulate, simulate_last_ms  # noqa: E402
from fleet_probe import models_of, timed  # noqa: E402

_dp = C.POINTER(C.c_double)


def fleet_shapes(a, lines):
    T, n = a.T, a.paths
    lib = _abi.load_library()
    base = {}
    for S in sorted({int(x) for x in a.series.split(",")} | (set() if a.no_baseline else {64}), key=lambda s: (s != 64, s)):
        ms = models_of("c2", S)
        keys = fleet_keys(FilterFleet.keys(cases.SEED, S))
        times = [0.5 * np.arange(1, T + 1)] * S
        with NativePfFleet(ms[0], 64, S) as fl:
            fl.set_params(ms)
            off, tt = fl.pack_times(times)
            t0 = np.zeros(S)
            ky = np.ascontiguousarray(keys, dtype=np.uint64)

            def call():
                _, rc = fl.simulate_packed(t0, off, tt, ky, n)
                assert not rc.any()
                return fl.simulate_last_ms()
            r = timed(call, a.repeats, a.warmup)
            if S == 64 and not a.no_baseline:
                descs = [m.descriptor() for m in ms]
                outs = [np.zeros((T + 1, ms[0].dimension + 3, n)) for _ in range(64)]
                tp = np.ascontiguousarray(times[0])

                def loop():
                    for k in range(64):
                        _abi.check(lib.cssm_simulate(descs[k].ptr(), n, keys[k], 0.0, tp.ctypes.data_as(_dp), T, 0, 0, outs[k].ctypes.data_as(_dp)))
                tl = [w for w, _ in timed(loop, a.spread, 1)]
                got, _ = fl.simulate_packed(t0, off, tt, ky, n)
                assert all(np.array_equal(got[k * (T + 1):(k + 1) * (T + 1)], outs[k]) for k in range(64))    # the same rows
                base["loop_ms_per_64"] = [round(x * 1e3, 3) for x in tl]
                base["loop_us_per_series"] = round(statistics.median(tl) / 64 * 1e6, 3)
                base["loop_spread_rel"] = round((max(tl) - min(tl)) / statistics.median(tl), 4)
        if str(S) not in a.series.split(","):
            continue
        wall = statistics.median(w for w, _ in r); dev = statistics.median(d for _, d in r)
        line = {"probe": "fleet_simulate", "model": "c2", "d": ms[0].dimension, "n_paths": n, "T": T, "S": S, "repeats": a.repeats,
                "wall_ms": round(wall * 1e3, 4), "device_ms": round(dev, 4), "wall_us_per_series": round(wall / S * 1e6, 4),
                "wall_min_ms": round(min(w for w, _ in r) * 1e3, 4), "wall_max_ms": round(max(w for w, _ in r) * 1e3, 4)}
        if base:
            line.update(base)
            line["loop_scaled_ms"] = round(statistics.median(base["loop_ms_per_64"]) * S / 64, 3)
            line["speedup_vs_loop"] = round(line["loop_scaled_ms"] / line["wall_ms"], 3)
        print(json.dumps(line), flush=True)
        lines.append(line)


def single_shape(a, lines):
    n, T = a.single_paths, a.single_T
    model = cases.c2_model()
    times = 0.5 * np.arange(1, T + 1)
    key = sim_key(cases.SEED)

    def sim():
        simulate(model, 0.0, times, n, key)
        return simulate_last_ms()
    r = timed(sim, a.single_repeats, 1)
    with NativePf(model, n, cases.SEED) as g:
        g.reseed(key)

        def fc():
            g.init(0.0)
            g.forecast(times, key, 0.975, want_samples=True)
            return g.forecast_last_ms()
        f = timed(fc, a.single_repeats, 1)
    line = {"probe": "simulate", "model": "c2", "d": model.dimension, "n_paths": n, "T": T, "repeats": a.single_repeats,
            "wall_ms": round(statistics.median(w for w, _ in r) * 1e3, 3), "k_simulate_ms": round(statistics.median(d for _, d in r), 4),
            "k_simulate_min_max_ms": [round(min(d for _, d in r), 4), round(max(d for _, d in r), 4)],
            "forecast_wall_ms": round(statistics.median(w for w, _ in f) * 1e3, 3),
            "k_forecast_ms": round(statistics.median(d[0] for _, d in f), 4),
            "k_forecast_min_max_ms": [round(min(d[0] for _, d in f), 4), round(max(d[0] for _, d in f), 4)],
            "forecast_select_ms": round(statistics.median(d[1] for _, d in f), 4)}
    line["rows_GB"] = round((T + 1) * (model.dimension + 3) * n * 8 / 1e9, 4)
    line["k_simulate_GB_per_s"] = round(line["rows_GB"] / (line["k_simulate_ms"] * 1e-3), 1)
    print(json.dumps(line), flush=True)
    lines.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", default="1024,16384")
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--paths", type=int, default=1, help="paths per series of the fleet shape")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--spread", type=int, default=5, help="repeats of the loop of single calls")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--no-fleet", action="store_true")
    ap.add_argument("--no-single", action="store_true")
    ap.add_argument("--single-paths", type=int, default=1 << 20)
    ap.add_argument("--single-T", type=int, default=24)
    ap.add_argument("--single-repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lines = []
    gc.disable()
    if not a.no_fleet:
        fleet_shapes(a, lines)
    if not a.no_single:
        single_shape(a, lines)
    gc.enable()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
