#!/usr/bin/env python3
"""fleet_interpolate_probe.py -- the fleet's interpolation (cssm_fleet_interpolate: FilterInterpolate of every series in two launches,
one workgroup per series forwards, one per (series, row) backwards) against what a fleet user had to do before it, in the same process
on the same GPU.  One JSON line per shape; the protocol of fleet_forecast_posterior_probe.py.

Shapes: model C2 (d = 3), N particles, S series, T records per series of which a block of --gap (a fraction) carries no observation.
Measured per shape: wall time around cssm_fleet_interpolate -- the records of all S x T observations built on the host included, it
ends in the stream's synchronise -- and the device time of its two launches (cssm_fleet_interpolate_last_ms), median of --repeats calls
after --warmup calls of the same shape, Python's collector off.  The ragged arrays are packed once outside the timed window.

Against (a): a loop of cssm_pf_interpolate calls on ONE reused NativePf of N particles (set_params + reseed per series), a series after
the other, the same data and keys.  64 series timed, --spread times, scaled linearly to S (exact for a sequential loop); the spread of
those repeats is the margin a fleet figure has to clear: the fleet wins when wall_ms < a_scaled_ms * (1 - a_spread_rel)."""
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
    ap.add_argument("--models", default="c2")
    ap.add_argument("--n", default="100,1000,4096")
    ap.add_argument("--series", default="1,64,1024")
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--gap", type=float, default=0.2, help="fraction of the records, in one block, without an observation")
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--spread", type=int, default=5, help="repeats of baseline (a)")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    T = a.T
    g0, g1 = T // 3, T // 3 + int(round(a.gap * T))
    lines = []
    gc.disable()
    for name in a.models.split(","):
        for n in (int(x) for x in a.n.split(",")):
            base = {}
            for S in sorted({int(x) for x in a.series.split(",")} | (set() if a.no_baseline else {64}), key=lambda s: (s != 64, s)):
                ms = models_of(name, S)
                seeds = FilterFleet.keys(cases.SEED, S)
                seven = {}
                datas = []
                for k in range(S):                                               # (seven distinct series, repeated)
                    if k % 7 not in seven:
                        t, y, has = cases.poisson_counts(T, seed=cases.SEED + k % 7)
                        has = has.copy(); has[g0:g1] = 0
                        seven[k % 7] = (t, y, has)
                    datas.append(seven[k % 7])
                with NativePfFleet(ms[0], n, S) as fl:
                    fl.set_params(ms); fl.reseed(seeds)
                    off, tt, yy, hh = fl.pack(datas)

                    def call():
                        _, _, rc = fl.interpolate_packed(off, tt, yy, hh)
                        assert not rc.any()
                        return fl.interpolate_last_ms()
                    r = timed(call, a.repeats, a.warmup)
                    if S == 64 and not a.no_baseline:
                        pf = NativePf(ms[0], n, seeds[0])

                        def loop_a():
                            for k in range(64):
                                pf.set_params(ms[k]); pf.reseed(seeds[k])
                                pf.interpolate(*datas[k])
                        ta = [w for w, _ in timed(loop_a, a.spread, 1)]
                        pf.close()
                        base["a_ms_per_64"] = [round(v * 1e3, 3) for v in ta]
                        base["a_ms_per_series"] = round(statistics.median(ta) / 64 * 1e3, 4)
                        base["a_spread_rel"] = round((max(ta) - min(ta)) / statistics.median(ta), 4)
                if str(S) not in a.series.split(","):
                    continue
                wall = statistics.median(w for w, _ in r)
                fwd = statistics.median(m[0] for _, m in r); lin = statistics.median(m[1] for _, m in r)
                line = {"probe": "fleet_interpolate", "model": name, "d": ms[0].dimension, "n": n, "T": T, "gap": [g0, g1], "S": S,
                        "repeats": a.repeats, "wall_ms": round(wall * 1e3, 4), "forward_ms": round(fwd, 4), "lineage_ms": round(lin, 4),
                        "wall_ms_per_series": round(wall / S * 1e3, 5), "device_ms_per_series": round((fwd + lin) / S, 5),
                        "wall_min_ms": round(min(w for w, _ in r) * 1e3, 4), "wall_max_ms": round(max(w for w, _ in r) * 1e3, 4)}
                if base:
                    line.update(base)
                    line["a_scaled_ms"] = round(statistics.median(base["a_ms_per_64"]) * S / 64, 3)
                    line["speedup_vs_a"] = round(line["a_scaled_ms"] / line["wall_ms"], 3)
                    line["fleet_below_a_by_more_than_its_spread"] = bool(line["wall_ms"] < line["a_scaled_ms"] * (1.0 - base["a_spread_rel"]))
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
