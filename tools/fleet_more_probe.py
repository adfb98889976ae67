#!/usr/bin/env python3
"""fleet_more_probe.py -- continuing a fleet by T records per series in ONE launch (cssm_fleet_ll_filter_more,
cssm_fleet_filter_intervals_more) against the only continuation a fleet had before them, the loop of cssm_fleet_step /
cssm_fleet_step_intervals: one launch, one upload, one read-back and one synchronisation per record.  The sibling of
fleet_intervals_probe.py, whose protocol this is.  ONE JSON line: {"probe": "fleet_more", "shapes": [one entry per shape]}.

Shapes: model C1 (d = 1) / C2 (d = 3), N particles, S series of T observations each.  Per repeat, on ONE fleet, the loop FIRST and the call
SECOND, each from the same start -- cssm_fleet_init_from of one state per series at the series' first time, outside the timed window:
  * the loop: T calls of cssm_fleet_step (cssm_fleet_step_intervals) on rows laid out once outside the timed window -- wall time, and the
    sum of the calls' device times (cssm_fleet_last_ms()[0] per record).  The loop's wall time holds NativePfFleet.step's array
    allocations, which favours the call: the device sums are stated next to it for that reason;
  * the call: cssm_fleet_ll_filter_more (cssm_fleet_filter_intervals_more) on arrays packed once outside the timed window -- wall time
    (it ends in the stream's synchronise) and device time (cssm_fleet_last_ms()[0]).
Both leave the same bits (tests/test_gpu_fleet_init_from.py); the probe asserts the final log-likelihoods equal.  gc is off across the
timed legs.  Median, min and max of --repeats repeats after --warmup of each; the loop's spread, (max - min) / median of its wall time, is
reported, and the call beats the loop when its median wall is below the loop's by more than that spread:
call_below_loop_by_more_than_its_spread.  A difference inside it shows nothing."""
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


def compare(loop, call):
    """one program's entry: the loop's and the call's wall and device times, the ratios, the verdict"""
    e = {"loop_wall_ms": stats([w for w, _ in loop], 1e3), "loop_device_ms": stats([d for _, d in loop]),
         "wall_ms": stats([w for w, _ in call], 1e3), "device_ms": stats([d for _, d in call])}
    lw, sp = e["loop_wall_ms"]["median"], e["loop_wall_ms"]["spread_rel"]
    e["speedup_vs_loop_wall"] = round(lw / e["wall_ms"]["median"], 3)
    e["speedup_vs_loop_device"] = round(e["loop_device_ms"]["median"] / e["device_ms"]["median"], 3)
    e["call_below_loop_by_more_than_its_spread"] = bool(e["wall_ms"]["median"] < lw * (1.0 - sp))
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="c2")
    ap.add_argument("--n", default="100,1000,4096")
    ap.add_argument("--series", default="1024")
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--interval", type=float, default=0.975)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    T = a.T
    shapes = []
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
                    rows = [np.full(fl.d, 0.1)] * S
                    last = {}

                    def start():
                        _, rc = fl.init_from(tm[0], rows)
                        assert not rc.any()

                    def loop(step):
                        dev = 0.0
                        t0 = time.perf_counter()
                        for r in range(T):
                            res = step(tm[r], ym[r], hm[r])
                            dev += fl.last_ms()[0]
                        w = time.perf_counter() - t0
                        assert not res[-1].any()
                        last["loop"] = res[0].copy()
                        return w, dev

                    def call(fn, *extra):
                        t0 = time.perf_counter()
                        res = fn(off, t, y, has, *extra)
                        w = time.perf_counter() - t0
                        assert not res[-1].any()
                        assert np.array_equal(res[0], last["loop"])          # the same bits, whichever way the records came
                        return w, fl.last_ms()[0]

                    legs = {"ll_filter_more": (lambda: loop(fl.step), lambda: call(fl.ll_filter_more_packed)),
                            "filter_intervals_more": (lambda: loop(lambda *r: fl.step_intervals(*r, interval=a.interval)),
                                                      lambda: call(fl.filter_intervals_more_packed, a.interval))}
                    got = {k: ([], []) for k in legs}
                    for rep in range(a.warmup + a.repeats):
                        for k, (lp, cl) in legs.items():                # the loop first, the call second, from the same start
                            start(); r_loop = lp()
                            start(); r_call = cl()
                            if rep >= a.warmup:
                                got[k][0].append(r_loop); got[k][1].append(r_call)
                shape = {"model": name, "d": ms[0].dimension, "n": n, "S": S, "T": T, "interval": a.interval, "repeats": a.repeats}
                for k in legs:
                    shape[k] = compare(*got[k])
                shapes.append(shape)
    gc.enable()
    line = json.dumps({"probe": "fleet_more", "shapes": shapes})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
