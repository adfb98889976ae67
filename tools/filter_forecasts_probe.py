#!/usr/bin/env python3
"""filter_forecasts_probe.py -- the single handle's one-step-ahead forecasts (cssm_pf_filter_forecasts: llFilter and getMeanForecast of
every record's time from the cloud before it, from ONE call) against what a user of one large cloud had to do before it, in the same
process on the same handle.  One JSON line per shape; the sibling of filter_intervals_probe.py, whose protocol this is.

Shapes: a model (--model c2 | bernoulli), T observations, N particles.  Per repeat, ALTERNATING on one handle:
  (a) call    cssm_pf_filter_forecasts -- wall time, and device time (cssm_pf_forecasts_last_ms: the whole call, its forecast rows alone);
  (b) loop    the route before it: cssm_pf_init, then per observation cssm_pf_forecast(H = 1) + cssm_pf_step -- wall time, and the device
              time of its forecasts (cssm_pf_forecast_last_ms: kernel + selection, summed over the records);
  (c) filter  cssm_pf_ll_filter alone -- wall time;
  (d) stream  cssm_pf_init, then cssm_pf_step_forecast per observation -- wall time, against (b).
Median, min and max of --repeats alternations after --warmup of each; the call beats the loop when its median wall is below the loop's by
more than the loop's own spread, (max - min) / median: call_below_loop_by_more_than_its_spread.  A difference inside it shows nothing.
row_device_us is the device time of one row's launches (the forecast kernel, the selection's passes, the finish): on a count-valued
observation row (Poisson: about ten distinct keys; Bernoulli: two) the selection's picked sub-range holds most of the row, so it reads
the keys again, up to CSSM_IV_ROUNDS times -- its worst case, and here the ordinary one; C2 against the Bernoulli model says what that costs."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="1000,100000,1048576")
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--model", default="c2", choices=("c2", "bernoulli"))
    ap.add_argument("--interval", type=float, default=0.975)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    T = a.T
    if a.model == "c2":
        model, (t, y, has) = cases.c2_model(), cases.poisson_counts(T)
    else:
        model, (t, y, has) = cases.bernoulli_model(), cases.binary_series(T)
    d = model.dimension
    t0 = float(np.min(t))
    lines = []
    gc.disable()
    for n in (int(x) for x in a.n.split(",")):
        with NativePf(model, n, cases.SEED) as g:
            def call():
                w0 = time.perf_counter()
                g.filter_forecasts(t, y, has, None, a.interval)
                w = time.perf_counter() - w0
                return (w,) + g.forecasts_last_ms()

            def loop():
                dev = 0.0
                w0 = time.perf_counter()
                g.init(t0)
                for s in range(T):
                    g.forecast([float(t[s])], None, a.interval)
                    dev += sum(g.forecast_last_ms())
                    g.step(float(t[s]), float(y[s]), bool(has[s]))
                return (time.perf_counter() - w0, dev)

            def ll_filter():
                w0 = time.perf_counter()
                g.run(t, y, has)
                return (time.perf_counter() - w0,)

            def stream():
                w0 = time.perf_counter()
                g.init(t0)
                for s in range(T):
                    g.step_forecast(float(t[s]), float(y[s]), bool(has[s]), None, a.interval)
                return (time.perf_counter() - w0,)

            fns = [("call", call), ("loop", loop), ("filter", ll_filter), ("stream", stream)]
            got = {k: [] for k, _ in fns}
            for rep in range(a.warmup + a.repeats):
                for k, fn in fns:                          # alternating: one of each per repeat
                    r = fn()
                    if rep >= a.warmup:
                        got[k].append(r)
        line = {"probe": "filter_forecasts", "model": a.model, "d": d, "n": n, "T": T, "interval": a.interval, "repeats": a.repeats,
                "call_wall_ms": stats([r[0] for r in got["call"]], 1e3), "call_device_ms": stats([r[1] for r in got["call"]]),
                "call_rows_device_ms": stats([r[2] for r in got["call"]]),
                "loop_wall_ms": stats([r[0] for r in got["loop"]], 1e3), "loop_forecasts_device_ms": stats([r[1] for r in got["loop"]]),
                "filter_wall_ms": stats([r[0] for r in got["filter"]], 1e3), "stream_wall_ms": stats([r[0] for r in got["stream"]], 1e3),
                "launches_per_row": 8, "launches_per_row_before": 18}
        cw, lw, sp = line["call_wall_ms"]["median"], line["loop_wall_ms"]["median"], line["loop_wall_ms"]["spread_rel"]
        line["speedup_vs_loop_wall"] = round(lw / cw, 3)
        line["call_below_loop_by_more_than_its_spread"] = bool(cw < lw * (1.0 - sp))
        line["row_wall_us_call_minus_filter"] = round((cw - line["filter_wall_ms"]["median"]) * 1e3 / T, 3)
        line["row_device_us"] = round(line["call_rows_device_ms"]["median"] * 1e3 / T, 3)
        line["row_device_us_loop"] = round(line["loop_forecasts_device_ms"]["median"] * 1e3 / T, 3)
        line["stream_speedup_vs_loop_wall"] = round(lw / line["stream_wall_ms"]["median"], 3)
        line["stream_below_loop_by_more_than_its_spread"] = bool(line["stream_wall_ms"]["median"] < lw * (1.0 - sp))
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
