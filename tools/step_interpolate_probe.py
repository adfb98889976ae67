#!/usr/bin/env python3
"""step_interpolate_probe.py -- the single handle's streaming interpolation (cssm_pf_window + cssm_pf_step_interpolate: cssm_pf_step and the
last lag + 1 time indices through the surviving lineages, per observation) against the only route a user of one large cloud had before it:
cssm_pf_step on one handle and, behind every observation, cssm_pf_interpolate of the whole prefix on a second.  One JSON line per shape; the
sibling of fleet_step_interpolate_probe.py and filter_intervals_probe.py, whose protocol this is.

Shapes: model C2 (d = 3), T observations, a window of --slices, --lag rows behind the newest, N particles.  Per repeat, ALTERNATING:
  (a) stream   cssm_pf_init, then cssm_pf_step_interpolate(lag) per observation -- wall time of the whole stream and of the call at the last
               record; in a pass of its own (stream_dev) the device times of every call (cssm_pf_step_interpolate_last_ms: the whole call,
               its row launches alone), added up, and those of the call at the last record;
      before   cssm_pf_step per observation on one handle and cssm_pf_interpolate of records 0 .. m on a second behind each -- wall time of
               the whole stream and of the pair at the last record (that call has no device timer: its device time stays unmeasured);
  (b) remember cssm_pf_step_interpolate(CSSM_PF_NO_ROWS) per observation -- wall time, and device time in stream_dev's manner -- against
      steps    the cssm_pf_step stream -- wall time;
  (c) one lineage row's device time (the last record's row launches / its rows) against one row of cssm_pf_step_intervals at the same N
      (cssm_pf_intervals_last_ms()[1]).
Median, min and max of --repeats alternations after --warmup of each; a route beats another when its median is below the other's by more
than the other's own spread, (max - min) / median.  A difference inside it shows nothing."""
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
from composablestatespacemodels_amd.filter import NativePf  # noqa: E402


def stats(v, scale=1.0, digits=4):
    v = [x * scale for x in v]
    med = statistics.median(v)
    return {"median": round(med, digits), "min": round(min(v), digits), "max": round(max(v), digits),
            "spread_rel": round((max(v) - min(v)) / med, 4) if med > 0 else None}


def below(a, b):
    """a's median below b's by more than b's own spread"""
    return bool(b["spread_rel"] is not None and a["median"] < b["median"] * (1.0 - b["spread_rel"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="1000,100000,1048576")
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--slices", type=int, default=16)
    ap.add_argument("--lag", type=int, default=10)
    ap.add_argument("--interval", type=float, default=0.975)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    T, lag = a.T, a.lag
    model = cases.c2_model()
    t, y, has = cases.poisson_counts(T)
    t0 = float(np.min(t))
    rec = [(float(t[s]), float(y[s]), bool(has[s])) for s in range(T)]
    lines = []
    gc.disable()
    for n in (int(x) for x in a.n.split(",")):
        with NativePf(model, n, cases.SEED) as g, NativePf(model, n, cases.SEED) as g2:
            g.window(a.slices)

            def stream(want_lag=lag):
                w0 = time.perf_counter()
                g.init(t0)
                for s in range(T - 1):
                    g.step_interpolate(*rec[s], lag=want_lag, interval=a.interval)
                w1 = time.perf_counter()
                g.step_interpolate(*rec[T - 1], lag=want_lag, interval=a.interval)
                w2 = time.perf_counter()
                return (w2 - w0, w2 - w1)

            def stream_dev(want_lag=lag):
                g.init(t0)
                whole = rows = 0.0
                for s in range(T):
                    _, _, nrows, _ = g.step_interpolate(*rec[s], lag=want_lag, interval=a.interval)
                    ms = g.step_interpolate_last_ms()
                    whole += ms[0]; rows += ms[1]
                return (whole, rows, ms[0], ms[1], nrows)

            def before():
                w0 = time.perf_counter()
                g.init(t0)
                for s in range(T):
                    w1 = time.perf_counter()
                    g.step(*rec[s])
                    g2.interpolate(t[:s + 1], y[:s + 1], has[:s + 1], a.interval)
                w2 = time.perf_counter()
                return (w2 - w0, w2 - w1)

            def steps():
                w0 = time.perf_counter()
                g.init(t0)
                for s in range(T):
                    g.step(*rec[s])
                return (time.perf_counter() - w0,)

            def intervals_row():
                g.init(t0)
                g.step(*rec[0])
                g.step_intervals(*rec[1], a.interval)
                return (g.intervals_last_ms()[1],)

            fns = [("stream", stream), ("stream_dev", stream_dev), ("before", before), ("remember", lambda: stream(None)),
                   ("remember_dev", lambda: stream_dev(None)), ("steps", steps), ("intervals_row", intervals_row)]
            got = {k: [] for k, _ in fns}
            for rep in range(a.warmup + a.repeats):
                for k, fn in fns:                          # alternating: one of each per repeat
                    r = fn()
                    if rep >= a.warmup:
                        got[k].append(r)
        nrows = int(got["stream_dev"][0][4])
        line = {"probe": "step_interpolate", "model": "c2", "d": model.dimension, "n": n, "T": T, "slices": a.slices, "lag": lag,
                "interval": a.interval, "repeats": a.repeats, "rows_at_last_record": nrows,
                "stream_wall_ms": stats([r[0] for r in got["stream"]], 1e3), "last_call_wall_ms": stats([r[1] for r in got["stream"]], 1e3),
                "stream_device_ms": stats([r[0] for r in got["stream_dev"]]), "stream_rows_device_ms": stats([r[1] for r in got["stream_dev"]]),
                "last_call_device_ms": stats([r[2] for r in got["stream_dev"]]), "last_call_rows_device_ms": stats([r[3] for r in got["stream_dev"]]),
                "before_stream_wall_ms": stats([r[0] for r in got["before"]], 1e3), "before_last_pair_wall_ms": stats([r[1] for r in got["before"]], 1e3),
                "before_device_ms": None,                 # (cssm_pf_interpolate has no device timer: unmeasured)
                "remember_wall_ms": stats([r[0] for r in got["remember"]], 1e3), "remember_device_ms": stats([r[0] for r in got["remember_dev"]]),
                "steps_wall_ms": stats([r[0] for r in got["steps"]], 1e3),
                "intervals_row_device_us": stats([r[0] for r in got["intervals_row"]], 1e3, 3)}
        line["lineage_row_device_us"] = stats([r[3] / max(r[4], 1) for r in got["stream_dev"]], 1e3, 3)
        line["stream_speedup_vs_before_wall"] = round(line["before_stream_wall_ms"]["median"] / line["stream_wall_ms"]["median"], 3)
        line["last_call_speedup_vs_before_wall"] = round(line["before_last_pair_wall_ms"]["median"] / line["last_call_wall_ms"]["median"], 3)
        line["stream_below_before_by_more_than_its_spread"] = below(line["stream_wall_ms"], line["before_stream_wall_ms"])
        line["last_call_below_before_by_more_than_its_spread"] = below(line["last_call_wall_ms"], line["before_last_pair_wall_ms"])
        line["remember_over_steps_wall"] = round(line["remember_wall_ms"]["median"] / line["steps_wall_ms"]["median"], 3)
        line["remember_us_per_record_over_steps"] = round((line["remember_wall_ms"]["median"] - line["steps_wall_ms"]["median"]) * 1e3 / T, 3)
        line["steps_below_remember_by_more_than_its_spread"] = below(line["steps_wall_ms"], line["remember_wall_ms"])
        line["lineage_row_over_intervals_row_device"] = round(line["lineage_row_device_us"]["median"] / line["intervals_row_device_us"]["median"], 3)
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
