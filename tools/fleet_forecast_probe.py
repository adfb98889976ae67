#!/usr/bin/env python3
"""fleet_forecast_probe.py -- the fleet's forecasts (cssm_fleet_forecast: every series' horizons in one launch, one workgroup per
series) against what a fleet user had to do before it, in the same process on the same GPU.  One JSON line per shape.

Shapes: model C1 (d = 1) / C2 (d = 3), N particles, S series, H horizons per series, from clouds that have seen T observations.
Measured per shape: wall time around cssm_fleet_forecast (it ends in the stream's synchronise) and the call's device time
(cssm_fleet_last_ms()[2]: HIP events around upload, launch and read-back), median of --repeats calls after warm-up calls of the same
shape, Python's collector off.  No samples are asked for; the ragged arrays are packed once (NativePfFleet.pack_times)
outside the timed window.

Against (a): ONE NativePf reused over the series -- per series set_params, reseed, init_from + adopt of the series' cloud (read back
from the fleet with cssm_fleet_get_particles OUTSIDE the timed window, which favours the baseline), then cssm_pf_forecast over the
same H times.  64 series timed, --spread times, scaled linearly to S (exact for a sequential loop); the spread of those repeats is the
margin a fleet figure has to clear.

Kernel times come from a run of their own under `rocprofv3 --kernel-trace --stats -- python tools/fleet_forecast_probe.py ...`."""
from __future__ import annotations

import argparse
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
from composablestatespacemodels_amd.filter import FilterFleet, NativePf, NativePfFleet  # noqa: E402
from fleet_probe import models_of, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="c1,c2")
    ap.add_argument("--n", default="100,1000,4096")
    ap.add_argument("--series", default="1,64,1024,4096")
    ap.add_argument("--H", type=int, default=24)
    ap.add_argument("--T", type=int, default=8, help="observations every cloud has seen before the forecast")
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--spread", type=int, default=5, help="repeats of baseline (a)")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--select", type=int, default=0, help="CSSM_OPT_FLEET_SELECT: 0 = by N, 1 = bitonic sort, 2 = radix select")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    H, T = a.H, a.T
    lines = []
    gc.disable()
    for name in a.models.split(","):
        for n in (int(x) for x in a.n.split(",")):
            base = {}
            for S in sorted({int(x) for x in a.series.split(",")} | (set() if a.no_baseline else {64}), key=lambda s: (s != 64, s)):
                ms = models_of(name, S)
                seeds = FilterFleet.keys(cases.SEED, S)
                packed = NativePfFleet.pack([cases.poisson_counts(T, seed=cases.SEED + k) for k in range(S)])
                times = [float(T - 1) + 0.5 * np.arange(1, H + 1)] * S
                with NativePfFleet(ms[0], n, S) as fl:
                    fl.set_params(ms); fl.reseed(seeds); fl.set_option(12, a.select)
                    _, _, _, rc = fl.ll_filter_packed(*packed)
                    assert not rc.any()
                    keys = [fl.forecast_key(k) for k in range(S)]
                    off, tt = fl.pack_times(times)
                    ky = np.ascontiguousarray(keys, dtype=np.uint64)

                    def call():
                        _, _, rc = fl.forecast_packed(off, tt, ky)
                        assert not rc.any()
                        return fl.last_ms()[2]
                    r = timed(call, a.repeats, a.warmup)
                    if S == 64 and not a.no_baseline:
                        # (a) one handle, the series one after the other, from the clouds the fleet holds
                        clouds = [fl.particles(k) for k in range(64)]
                        pf = NativePf(ms[0], n, seeds[0])

                        def loop_a():
                            for k in range(64):
                                pf.set_params(ms[k]); pf.reseed(seeds[k])
                                pf.init_from(float(T - 1), clouds[k][:, 0]); pf.adopt(clouds[k], 0.0, n)
                                pf.forecast(times[k], keys[k])
                        ta = [w for w, _ in timed(loop_a, a.spread, 1)]
                        pf.close()
                        base["a_ms_per_64"] = [round(x * 1e3, 3) for x in ta]
                        base["a_us_per_series_horizon"] = round(statistics.median(ta) / (64 * H) * 1e6, 3)
                        base["a_spread_rel"] = round((max(ta) - min(ta)) / statistics.median(ta), 4)
                if str(S) not in a.series.split(","):
                    continue
                wall = statistics.median(w for w, _ in r); dev = statistics.median(d for _, d in r)
                line = {"probe": "fleet_forecast", "model": name, "d": ms[0].dimension, "n": n, "H": H, "S": S, "repeats": a.repeats, "select": a.select,
                        "wall_ms": round(wall * 1e3, 4), "device_ms": round(dev, 4),
                        "wall_us_per_series_horizon": round(wall / (S * H) * 1e6, 4),
                        "device_us_per_series_horizon": round(dev * 1e3 / (S * H), 4),
                        "wall_min_ms": round(min(w for w, _ in r) * 1e3, 4), "wall_max_ms": round(max(w for w, _ in r) * 1e3, 4)}
                if base:
                    line.update(base)
                    line["a_scaled_ms"] = round(statistics.median(base["a_ms_per_64"]) * S / 64, 3)
                    line["speedup_vs_a"] = round(line["a_scaled_ms"] / line["wall_ms"], 3)
                print(json.dumps(line), flush=True)
                lines.append(line)
    gc.enable()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        order = a.models.split(",")
        with open(a.out, "w") as f:
            for line in sorted(lines, key=lambda l: (order.index(l["model"]), l["n"], l["S"])):
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
