#!/usr/bin/env python3
"""fleet_probe.py -- the fleet filter (cssm_fleet_*: S small series per launch, one workgroup each) against what a user with S
series could do before it, in the same process on the same GPU.  One JSON line per shape.

Shapes: model C1 (d = 1) / C2 (d = 3), N particles, T observations, S series (state memory S N d 16 bytes).
Measured per shape: wall time around cssm_fleet_ll_filter (it ends in the stream's synchronise) and the call's device time
(cssm_fleet_last_ms: HIP events around upload, launch and read-back), median of --repeats calls after warm-up calls of the same
shape, Python's collector off.  The arrays are packed once (NativePfFleet.pack) outside the timed window.

Against:
  (a) one NativePf reused over the series (set_params, reseed, run): 64 series timed, --spread times, scaled linearly to S (exact for
      a sequential loop); the spread of those repeats is the margin a fleet figure has to clear;
  (b) where the series share t / y / has (the pilot-run shape): NativePfBatch with 64 chains, ceil(S / 64) calls.

Kernel times come from a run of their own under `rocprofv3 --kernel-trace --stats -- python tools/fleet_probe.py ...`."""
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

import cases  # noqa: E402
from composablestatespacemodels_amd.filter import FilterFleet, NativePf, NativePfBatch, NativePfFleet  # noqa: E402


def perturbed(make_params, k):
    p = make_params()
    th = np.asarray(p.flattenParams())
    return p.withFlat(th + 0.03 * (k % 7) * np.cos(np.arange(th.size) + k))


def models_of(name, count):
    """`count` parameter sets of one structure (seven distinct ones, repeated)"""
    if name == "c1":
        return [cases.c1_model()] * count
    um = cases.c2_unparam()
    seven = [um.run(perturbed(cases.c2_params, k)) for k in range(7)]
    return [seven[k % 7] for k in range(count)]


def timed(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        extra = fn()
        out.append((time.perf_counter() - t0, extra))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="c1,c2")
    ap.add_argument("--n", default="100,1000,4096")
    ap.add_argument("--series", default="1,64,1024,4096,16384")
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--spread", type=int, default=5, help="repeats of baseline (a)")
    ap.add_argument("--no-baselines", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    T = a.T
    lines = []
    gc.disable()
    for name in a.models.split(","):
        for n in (int(x) for x in a.n.split(",")):
            keys = FilterFleet.keys(cases.SEED, 64)
            ms64 = models_of(name, 64)
            datas64 = [cases.poisson_counts(T, seed=cases.SEED + k) for k in range(64)]
            base = {}
            if not a.no_baselines:
                # (a) one handle, the series one after the other
                pf = NativePf(ms64[0], n, keys[0])

                def loop_a():
                    for k in range(64):
                        pf.set_params(ms64[k]); pf.reseed(keys[k]); pf.run(*datas64[k])
                ta = [w for w, _ in timed(loop_a, a.spread, 1)]
                pf.close()
                base["a_ms_per_64"] = [round(x * 1e3, 3) for x in ta]
                base["a_us_per_series_obs"] = round(statistics.median(ta) / (64 * T) * 1e6, 3)
                base["a_spread_rel"] = round((max(ta) - min(ta)) / statistics.median(ta), 4)
                # (b) the batch: 64 chains on shared data
                b = NativePfBatch(ms64[0], n, 64)
                tb = [w for w, _ in timed(lambda: b.filter(ms64, keys, *datas64[0], want_path=False), a.spread, 1)]
                b.close()
                base["b_ms_per_64"] = [round(x * 1e3, 3) for x in tb]
                base["b_us_per_series_obs"] = round(statistics.median(tb) / (64 * T) * 1e6, 3)
            for S in (int(x) for x in a.series.split(",")):
                if S * n * cases.c2_model().dimension * 16 > 24 << 30:
                    continue
                ms = models_of(name, S)
                seeds = FilterFleet.keys(cases.SEED, S)
                packed = NativePfFleet.pack([cases.poisson_counts(T, seed=cases.SEED + k) for k in range(S)])
                with NativePfFleet(ms[0], n, S) as fl:
                    fl.set_params(ms); fl.reseed(seeds)

                    def call():
                        _, _, _, rc = fl.ll_filter_packed(*packed)
                        assert not rc.any()
                        return fl.last_ms()[0]
                    r = timed(call, a.repeats, a.warmup)
                wall = statistics.median(w for w, _ in r); dev = statistics.median(d for _, d in r)
                line = {"probe": "fleet", "model": name, "d": ms[0].dimension, "n": n, "T": T, "S": S, "repeats": a.repeats,
                        "wall_ms": round(wall * 1e3, 4), "device_ms": round(dev, 4),
                        "wall_us_per_series_obs": round(wall / (S * T) * 1e6, 4), "device_us_per_series_obs": round(dev * 1e3 / (S * T), 4),
                        "wall_min_ms": round(min(w for w, _ in r) * 1e3, 4), "wall_max_ms": round(max(w for w, _ in r) * 1e3, 4)}
                if base:
                    line.update(base)
                    line["a_scaled_ms"] = round(statistics.median(base["a_ms_per_64"]) * S / 64, 3)
                    line["speedup_vs_a"] = round(line["a_scaled_ms"] / line["wall_ms"], 3)
                    line["b_scaled_ms"] = round(statistics.median(base["b_ms_per_64"]) * -(-S // 64), 3)
                    line["speedup_vs_b"] = round(line["b_scaled_ms"] / line["wall_ms"], 3)
                print(json.dumps(line), flush=True)
                lines.append(line)
    gc.enable()
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
