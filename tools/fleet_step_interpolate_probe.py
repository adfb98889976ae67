#!/usr/bin/env python3
"""fleet_step_interpolate_probe.py -- the fleet's streaming interpolation (cssm_fleet_step_interpolate: one observation per sensor per
call, every cloud remembered in a window on the device, the last lag + 1 time indices summarised through the surviving lineages by a
second launch) against what a fleet user had to do before it, in the same process on the same fleet.  One JSON line per shape; the
protocol of fleet_interpolate_probe.py and fleet_intervals_probe.py.

Shapes: model C1 (d = 1) / C2 (d = 3), N particles, S series of T observations each, a window of --slices, rows of --lag.  Per repeat,
ALTERNATING on one fleet, every leg from cssm_fleet_init:
  * stream_rows: T calls of step_interpolate with lag = --lag -- (c), the new way; its last call (record T - 1) is (a)'s;
  * stream_quiet: T calls with every series at CSSM_FLEET_NO_ROWS -- (b): one launch each, the price of remembering;
  * steps: T calls of cssm_fleet_step -- (b)'s baseline; behind its last step cssm_fleet_interpolate of the whole T-record prefix on
    arrays packed outside the timed window: step + interpolate is (a)'s baseline, the only way to those rows before;
  * stream_prefix (unless --no-prefix-stream): per record cssm_fleet_step + cssm_fleet_interpolate of the prefix so far -- (c)'s baseline,
    O(m) records forward and O(m) row sorts backward for the m-th record.
Wall time per call ends in the stream's synchronise and holds the Python wrappers' array allocations on both sides; device time is
cssm_fleet_last_ms()[0] (a step call, both of its launches) and cssm_fleet_interpolate_last_ms() (the two launches, summed).
Median, min and max of --repeats alternations after --warmup of each.  A ratio is claimed only where the new figure lies outside the
baseline's own spread, (max - min) / median: *_beyond_baseline_spread.  A difference inside it shows nothing."""
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


def compare(line, key, new, base):
    """new / base figures (stats dicts): the ratio of the medians, and whether the new median lies outside the baseline's spread"""
    b, sp = base["median"], base["spread_rel"] or 0.0
    line[key + "_ratio_base_over_new"] = round(b / new["median"], 3) if new["median"] > 0 else None
    line[key + "_beyond_baseline_spread"] = bool(new["median"] < b * (1.0 - sp) or new["median"] > b * (1.0 + sp))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="c2")
    ap.add_argument("--n", default="1000")
    ap.add_argument("--series", default="1024")
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--lag", type=int, default=10)
    ap.add_argument("--slices", type=int, default=16)
    ap.add_argument("--interval", type=float, default=0.975)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-prefix-stream", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
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
                tm = np.ascontiguousarray(np.stack([d[0] for d in datas], axis=1))      # [T][S]: a call's rows
                ym = np.ascontiguousarray(np.stack([d[1] for d in datas], axis=1))
                hm = np.ascontiguousarray(np.stack([d[2] for d in datas], axis=1))
                quiet = np.full(S, 0xFFFFFFFF, dtype=np.uint32)          # CSSM_FLEET_NO_ROWS for every series
                with NativePfFleet(ms[0], n, S) as fl:
                    fl.set_params(ms); fl.reseed(seeds)
                    fl.window(a.slices)
                    packed = {m: fl.pack([(d[0][:m], d[1][:m], d[2][:m]) for d in datas]) for m in ([T] if a.no_prefix_stream else range(1, T + 1))}

                    def stream(lag):
                        """T step_interpolate calls: (wall of the stream, device of the stream, wall of the last call, device of it,
                        the lineage launch's share of it)"""
                        fl.init(tm[0])
                        wall = dev = 0.0
                        for r in range(T):
                            t0 = time.perf_counter()
                            _, _, _, _, rc = fl.step_interpolate(tm[r], ym[r], hm[r], None, lag, a.lag, a.interval)
                            w = time.perf_counter() - t0
                            d = fl.last_ms()[0]
                            wall += w; dev += d
                        assert not rc.any()
                        return wall, dev, w, d, fl.step_interpolate_last_ms()[1]

                    def interp(m):
                        t0 = time.perf_counter()
                        _, _, rc = fl.interpolate_packed(*packed[m], interval=a.interval)
                        w = time.perf_counter() - t0
                        assert not rc.any()
                        return w, sum(fl.interpolate_last_ms())

                    def steps(every):
                        """T cssm_fleet_step calls, cssm_fleet_interpolate of the prefix behind every one (every) or behind the last:
                        (wall of the steps, device of them, wall of the last step, device of it, wall of the interpolations, device)"""
                        fl.init(tm[0])
                        wall = dev = iw = idv = 0.0
                        for r in range(T):
                            t0 = time.perf_counter()
                            _, _, rc = fl.step(tm[r], ym[r], hm[r])
                            w = time.perf_counter() - t0
                            d = fl.last_ms()[0]
                            wall += w; dev += d
                            if every or r == T - 1:
                                x, y = interp(r + 1)
                                iw += x; idv += y
                        assert not rc.any()
                        return wall, dev, w, d, iw, idv

                    fns = [("rows", lambda: stream(None)), ("quiet", lambda: stream(quiet)), ("steps", lambda: steps(False))]
                    if not a.no_prefix_stream:
                        fns.append(("prefix", lambda: steps(True)))
                    got = {k: [] for k, _ in fns}
                    for rep in range(a.warmup + a.repeats):
                        for k, fn in fns:                          # alternating: one of each per repeat
                            r = fn()
                            if rep >= a.warmup:
                                got[k].append(r)
                col = lambda k, i, j=None: [(r[i] + (r[j] if j is not None else 0.0)) for r in got[k]]
                line = {"probe": "fleet_step_interpolate", "model": name, "d": ms[0].dimension, "n": n, "S": S, "T": T, "lag": a.lag,
                        "slices": a.slices, "interval": a.interval, "repeats": a.repeats,
                        "window_bytes": S * a.slices * n * (8 * ms[0].dimension + 4),
                        # (a) the call at record T - 1 with rows | step + interpolate of the T-record prefix
                        "a_call_wall_ms": stats(col("rows", 2), 1e3), "a_call_device_ms": stats(col("rows", 3)),
                        "a_call_lineage_device_ms": stats(col("rows", 4)),
                        "a_base_wall_ms": stats(col("steps", 2, 4), 1e3), "a_base_device_ms": stats(col("steps", 3, 5)),
                        # (b) T calls without rows | T plain steps
                        "b_quiet_wall_ms": stats(col("quiet", 0), 1e3), "b_quiet_device_ms": stats(col("quiet", 1)),
                        "b_steps_wall_ms": stats(col("steps", 0), 1e3), "b_steps_device_ms": stats(col("steps", 1)),
                        # (c) the whole stream with rows
                        "c_stream_wall_ms": stats(col("rows", 0), 1e3), "c_stream_device_ms": stats(col("rows", 1))}
                compare(line, "a_wall", line["a_call_wall_ms"], line["a_base_wall_ms"])
                compare(line, "a_device", line["a_call_device_ms"], line["a_base_device_ms"])
                compare(line, "b_wall", line["b_quiet_wall_ms"], line["b_steps_wall_ms"])
                compare(line, "b_device", line["b_quiet_device_ms"], line["b_steps_device_ms"])
                line["b_remember_device_us_per_record"] = round(
                    (line["b_quiet_device_ms"]["median"] - line["b_steps_device_ms"]["median"]) * 1e3 / (S * T), 4)
                if not a.no_prefix_stream:
                    line["c_base_wall_ms"] = stats(col("prefix", 0, 4), 1e3)
                    line["c_base_device_ms"] = stats(col("prefix", 1, 5))
                    compare(line, "c_wall", line["c_stream_wall_ms"], line["c_base_wall_ms"])
                    compare(line, "c_device", line["c_stream_device_ms"], line["c_base_device_ms"])
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
