#!/usr/bin/env python3
"""fleet_forecast_posterior_probe.py -- the fleet's posterior-predictive forecasts (cssm_fleet_forecast_posterior: every series' horizons
under its own joint posterior sample in one launch, one workgroup per series) against what a fleet user had to do before it, in the
same process on the same GPU.  One JSON line per shape; the sibling of fleet_forecast_probe.py, whose protocol this is.

Shapes: model C1 (d = 1) / C2 (d = 3), N particles, S series, H horizons per series, M posterior pairs per series (rows around the
series' own parameters, as tests/test_gpu_forecast_posterior.py draws them).  Measured per shape: wall time around
cssm_fleet_forecast_posterior -- the validation and constraint transform of all S x M rows on the host included, it ends in the stream's
synchronise -- and the call's device time (cssm_fleet_last_ms()[2]), median of --repeats calls after warm-up calls of the same shape,
Python's collector off.  No samples are asked for; the ragged arrays are packed once outside the timed window, as in the sibling probe --
which favours the fleet, since baseline (a) pays NativePf.forecast_posterior's conversions and allocations per call: wall_packing_ms is
the same call with pack_posteriors and pack_times inside the window, and the condition is stated for both.

Against (a): a loop of cssm_pf_forecast_posterior calls on ONE reused NativePf of N particles, a series after the other, the same rows,
times and keys.  64 series timed, --spread times, scaled linearly to S (exact for a sequential loop); the spread of those repeats is the
margin a fleet figure has to clear: the fleet wins when wall_ms < a_scaled_ms * (1 - a_spread_rel)."""
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
from composablestatespacemodels_amd.model import Parameters  # noqa: E402
from fleet_probe import models_of, timed  # noqa: E402


def posterior_of(model, M, seed, spread=0.25):
    rng = np.random.default_rng(seed)
    th0 = np.asarray(Parameters([node for _, node, _ in model.leaves]).flattenParams())
    d = sum(sde.dimension for _, _, sde in model.leaves)
    return th0 + spread * rng.standard_normal((M, th0.size)), 0.5 * rng.standard_normal((M, d))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="c2")
    ap.add_argument("--n", default="1000")
    ap.add_argument("--series", default="1024")
    ap.add_argument("--H", type=int, default=24)
    ap.add_argument("--posterior", type=int, default=1000, help="M: posterior pairs per series")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--spread", type=int, default=5, help="repeats of baseline (a)")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--select", type=int, default=0, help="CSSM_OPT_FLEET_SELECT: 0 = by N, 1 = bitonic sort, 2 = radix select")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    H, M, t0 = a.H, a.posterior, 7.0
    lines = []
    gc.disable()
    for name in a.models.split(","):
        for n in (int(x) for x in a.n.split(",")):
            base = {}
            for S in sorted({int(x) for x in a.series.split(",")} | (set() if a.no_baseline else {64}), key=lambda s: (s != 64, s)):
                ms = models_of(name, S)
                seeds = FilterFleet.keys(cases.SEED, S)
                seven = {}
                post = [seven.setdefault(k % 7, posterior_of(ms[k], M, 3 + k % 7)) for k in range(S)]      # (seven distinct samples, repeated)
                times = [t0 + 0.5 * np.arange(1, H + 1)] * S
                with NativePfFleet(ms[0], n, S) as fl:
                    fl.set_params(ms); fl.reseed(seeds); fl.set_option(12, a.select)
                    keys = [fl.posterior_key(k) for k in range(S)]
                    moff, theta, x = fl.pack_posteriors(post)
                    off, tt = fl.pack_times(times)
                    t0s = np.full(S, t0)
                    ky = np.ascontiguousarray(keys, dtype=np.uint64)

                    def call():
                        _, _, _, rc = fl.forecast_posterior_packed(moff, theta, x, t0s, off, tt, ky)
                        assert not rc.any()
                        return fl.last_ms()[2]
                    r = timed(call, a.repeats, a.warmup)

                    def call_packing():
                        m2, th2, x2 = fl.pack_posteriors(post)
                        o2, t2 = fl.pack_times(times)
                        _, _, _, rc = fl.forecast_posterior_packed(m2, th2, x2, t0s, o2, t2, ky)
                        assert not rc.any()
                    rp = timed(call_packing, a.repeats, 0)
                    if S == 64 and not a.no_baseline:
                        pf = NativePf(ms[0], n, seeds[0])

                        def loop_a():
                            for k in range(64):
                                pf.forecast_posterior(post[k][0], post[k][1], t0, times[k], keys[k])
                        ta = [w for w, _ in timed(loop_a, a.spread, 1)]
                        pf.close()
                        base["a_ms_per_64"] = [round(v * 1e3, 3) for v in ta]
                        base["a_us_per_series_horizon"] = round(statistics.median(ta) / (64 * H) * 1e6, 3)
                        base["a_spread_rel"] = round((max(ta) - min(ta)) / statistics.median(ta), 4)
                if str(S) not in a.series.split(","):
                    continue
                wall = statistics.median(w for w, _ in r); dev = statistics.median(d for _, d in r)
                line = {"probe": "fleet_forecast_posterior", "model": name, "d": ms[0].dimension, "n": n, "H": H, "M": M, "S": S,
                        "repeats": a.repeats, "select": a.select, "wall_ms": round(wall * 1e3, 4), "device_ms": round(dev, 4),
                        "wall_us_per_series_horizon": round(wall / (S * H) * 1e6, 4),
                        "device_us_per_series_horizon": round(dev * 1e3 / (S * H), 4),
                        "wall_min_ms": round(min(w for w, _ in r) * 1e3, 4), "wall_max_ms": round(max(w for w, _ in r) * 1e3, 4)}
                line["wall_packing_ms"] = round(statistics.median(w for w, _ in rp) * 1e3, 4)
                if base:
                    line.update(base)
                    line["a_scaled_ms"] = round(statistics.median(base["a_ms_per_64"]) * S / 64, 3)
                    line["speedup_vs_a"] = round(line["a_scaled_ms"] / line["wall_ms"], 3)
                    line["fleet_below_a_by_more_than_its_spread"] = bool(line["wall_ms"] < line["a_scaled_ms"] * (1.0 - base["a_spread_rel"]))
                    line["speedup_vs_a_with_packing"] = round(line["a_scaled_ms"] / line["wall_packing_ms"], 3)
                    line["fleet_with_packing_below_a_by_more_than_its_spread"] = bool(
                        line["wall_packing_ms"] < line["a_scaled_ms"] * (1.0 - base["a_spread_rel"]))
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
