#!/usr/bin/env python3
"""fleet_filter_forecasts_probe.py -- the fleet's one-step-ahead forecasts (cssm_fleet_filter_forecasts: every series' llFilter and,
before every record is weighed, the forecast of its time from the cloud before it, in ONE launch, one workgroup per series) against what
a fleet user had to do before it, in the same process on the same fleet.  One JSON line per shape; the protocol of
fleet_intervals_probe.py.

Shapes: model C1 (d = 1) / C2 (d = 3), N particles, S series of T observations each.  Per repeat, ALTERNATING on one fleet:
  * the call: cssm_fleet_filter_forecasts on arrays packed once outside the timed window, default keys -- wall time (it ends in the
    stream's synchronise) and device time (cssm_fleet_last_ms()[0]);
  * the loop, which is the parent commit's path: cssm_fleet_init at the series' first times, then per observation cssm_fleet_forecast
    with one horizon per series (arrays and keys made outside the timed window) + cssm_fleet_step -- 2 T launches, uploads, read-backs
    and synchronisations; wall time, and the sum of the calls' device times (cssm_fleet_last_ms()[2] + [0] per observation).  The
    loop's wall time holds the Python wrapper's array allocations of 2 T calls, which favours the call: the device sums are stated
    next to it for that reason;
  * for context, cssm_fleet_filter_intervals on the same arrays (the same d + 1 row sorts per record, one row and the extra propagate
    fewer) and cssm_fleet_ll_filter (the price of the forecasts per record in device time, (device_ms - ll_filter_device_ms) / (S T)).
Median, min and max of --repeats (at least 7) alternations after --warmup of each; the call beats the loop when its median wall is
below the loop's by more than the loop's own spread, (max - min) / median: call_below_loop_by_more_than_its_spread.  A difference inside
it shows nothing."""
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
from composablestatespacemodels_amd.filter import FilterFleet, NativePfFleet  # noqa: E402
from fleet_probe import models_of  # noqa: E402


def stats(v, scale=1.0, digits=4):
    v = [x * scale for x in v]
    med = statistics.median(v)
    return {"median": round(med, digits), "min": round(min(v), digits), "max": round(max(v), digits),
            "spread_rel": round((max(v) - min(v)) / med, 4) if med > 0 else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="c2")
    ap.add_argument("--n", default="100,1000,4096")
    ap.add_argument("--series", default="1024")
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--interval", type=float, default=0.975)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.repeats < 7:
        ap.error("at least 7 repeats")
    T = a.T
    lines = []
    gc.disable()
    for name in a.models.split(","):
        for n in (int(x) for x in a.n.split(",")):
            for S in (int(x) for x in a.series.split(",")):
                ms = models_of(name, S)
                seeds = FilterFleet.keys(cases.SEED, S)
                seven = [cases.poisson_counts(T, seed=cases.SEED + k) for k in range(7)]
                datas = [seven[k % 7] for k in range(S)]
                tm = np.ascontiguousarray(np.stack([d[0] for d in datas], axis=1))      # [T][S]: the loop's rows
                ym = np.ascontiguousarray(np.stack([d[1] for d in datas], axis=1))
                hm = np.ascontiguousarray(np.stack([d[2] for d in datas], axis=1))
                with NativePfFleet(ms[0], n, S) as fl:
                    fl.set_params(ms); fl.reseed(seeds)
                    off, t, y, has = fl.pack(datas)
                    one = np.arange(S + 1, dtype=np.uint64)                      # the loop's forecasts: one horizon per series
                    lib = fl.lib                                                 # ... under the keys the call takes by default
                    fkeys = np.ascontiguousarray([[lib.cssm_pf_run_key(int(seeds[k]), (1 << 63) | r) for k in range(S)] for r in range(T)],
                                                 dtype=np.uint64)

                    def call():
                        t0 = time.perf_counter()
                        _, _, _, _, rc, fc_rc = fl.filter_forecasts_packed(off, t, y, has, a.interval)
                        w = time.perf_counter() - t0
                        assert not rc.any() and not fc_rc.any()
                        return w, fl.last_ms()[0]

                    def intervals():
                        t0 = time.perf_counter()
                        _, _, _, _, rc = fl.filter_intervals_packed(off, t, y, has, a.interval)
                        w = time.perf_counter() - t0
                        assert not rc.any()
                        return w, fl.last_ms()[0]

                    def ll_filter():
                        t0 = time.perf_counter()
                        _, _, _, rc = fl.ll_filter_packed(off, t, y, has)
                        w = time.perf_counter() - t0
                        assert not rc.any()
                        return w, fl.last_ms()[0]

                    def loop():
                        dev = 0.0
                        t0 = time.perf_counter()
                        fl.init(tm[0])
                        for r in range(T):
                            _, _, frc = fl.forecast_packed(one, tm[r], fkeys[r], a.interval)
                            f_ms = fl.last_ms()[2]
                            _, _, rc = fl.step(tm[r], ym[r], hm[r])
                            dev += f_ms + fl.last_ms()[0]
                            assert not frc.any()
                        w = time.perf_counter() - t0
                        assert not rc.any()
                        return w, dev

                    fns = [("call", call), ("intervals", intervals), ("ll_filter", ll_filter)] + ([] if a.no_baseline else [("loop", loop)])
                    got = {k: [] for k, _ in fns}
                    for rep in range(a.warmup + a.repeats):
                        for k, fn in fns:                          # alternating: one of each per repeat
                            r = fn()
                            if rep >= a.warmup:
                                got[k].append(r)
                line = {"probe": "fleet_filter_forecasts", "model": name, "d": ms[0].dimension, "n": n, "S": S, "T": T, "interval": a.interval,
                        "repeats": a.repeats,
                        "wall_ms": stats([w for w, _ in got["call"]], 1e3), "device_ms": stats([d for _, d in got["call"]]),
                        "filter_intervals_wall_ms": stats([w for w, _ in got["intervals"]], 1e3),
                        "filter_intervals_device_ms": stats([d for _, d in got["intervals"]]),
                        "ll_filter_wall_ms": stats([w for w, _ in got["ll_filter"]], 1e3),
                        "ll_filter_device_ms": stats([d for _, d in got["ll_filter"]])}
                line["forecasts_device_us_per_record"] = round(
                    (line["device_ms"]["median"] - line["ll_filter_device_ms"]["median"]) * 1e3 / (S * T), 4)
                line["wall_us_per_record"] = round(line["wall_ms"]["median"] * 1e3 / (S * T), 4)
                if not a.no_baseline:
                    line["loop_wall_ms"] = stats([w for w, _ in got["loop"]], 1e3)
                    line["loop_device_ms"] = stats([d for _, d in got["loop"]])
                    lw, sp = line["loop_wall_ms"]["median"], line["loop_wall_ms"]["spread_rel"]
                    line["speedup_vs_loop_wall"] = round(lw / line["wall_ms"]["median"], 3)
                    line["speedup_vs_loop_device"] = round(line["loop_device_ms"]["median"] / line["device_ms"]["median"], 3)
                    line["call_below_loop_by_more_than_its_spread"] = bool(line["wall_ms"]["median"] < lw * (1.0 - sp))
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
