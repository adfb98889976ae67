#!/usr/bin/env python3
"""filter_intervals_probe.py -- the single handle's filtered intervals (cssm_pf_filter_intervals: llFilter and getIntervals of the cloud
behind every observation from ONE call) against what a user of one large cloud had to do before it, in the same process on the same
handle.  One JSON line per shape; the sibling of fleet_intervals_probe.py, whose protocol this is.

Shapes: model C2 (d = 3), T observations, N particles.  Per repeat, ALTERNATING on one handle:
  (a) call    cssm_pf_filter_intervals -- wall time, and device time (cssm_pf_intervals_last_ms: the whole call, its summary launches alone);
  (b) loop    the route before it: cssm_pf_init, cssm_pf_summary, then per observation cssm_pf_step + cssm_pf_summary -- wall time;
  (c) filter  cssm_pf_ll_filter alone -- wall time;
  (d) steps   cssm_pf_init and the cssm_pf_step stream alone -- wall time: (b) - (d) is what the loop pays for its T + 1 summaries;
  (e) stream  cssm_pf_init, cssm_pf_summary, then cssm_pf_step_intervals per observation -- wall time, against (b).
Median, min and max of --repeats alternations after --warmup of each; the call beats the loop when its median wall is below the loop's by
more than the loop's own spread, (max - min) / median: call_below_loop_by_more_than_its_spread.  A difference inside it shows nothing.
Counted, not measured: the launches of a row (the fill, the enqueued passes, the finish), the reads of the cloud or its keys a row of
the final cloud takes (the sequential twin tests/cpp/intervals_twin.c on every state row: 1 + its passes over the keys), and from them the
row's bytes (cloud + ancestors read, keys written, keys read that many times), whose rate over the summaries' device time per row is
stated as a share of cssm_diag_copy_ceiling on the same device."""
from __future__ import annotations

import argparse
import ctypes as C
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
from composablestatespacemodels_amd import _abi  # noqa: E402
from composablestatespacemodels_amd.filter import NativePf  # noqa: E402
from test_filter_intervals_host import twin_constants, twin_select  # noqa: E402


def stats(v, scale=1.0, digits=4):
    v = [x * scale for x in v]
    med = statistics.median(v)
    return {"median": round(med, digits), "min": round(min(v), digits), "max": round(max(v), digits),
            "spread_rel": round((max(v) - min(v)) / med, 4) if med > 0 else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="1000,100000,1048576")
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--interval", type=float, default=0.975)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    T = a.T
    model = cases.c2_model()
    d = model.dimension
    t, y, has = cases.poisson_counts(T)
    t0 = float(np.min(t))
    gbps = C.c_double()
    _abi.check(_abi.load_library().cssm_diag_copy_ceiling(0, 1 << 30, 5, C.byref(gbps)))
    lines = []
    gc.disable()
    for n in (int(x) for x in a.n.split(",")):
        with NativePf(model, n, cases.SEED) as g:
            def call():
                w0 = time.perf_counter()
                g.filter_intervals(t, y, has, a.interval)
                w = time.perf_counter() - w0
                return (w,) + g.intervals_last_ms()

            def loop():
                w0 = time.perf_counter()
                g.init(t0); g.summary(a.interval)
                for s in range(T):
                    g.step(float(t[s]), float(y[s]), bool(has[s])); g.summary(a.interval)
                return (time.perf_counter() - w0,)

            def ll_filter():
                w0 = time.perf_counter()
                g.run(t, y, has)
                return (time.perf_counter() - w0,)

            def steps():
                w0 = time.perf_counter()
                g.init(t0)
                for s in range(T):
                    g.step(float(t[s]), float(y[s]), bool(has[s]))
                return (time.perf_counter() - w0,)

            def stream():
                w0 = time.perf_counter()
                g.init(t0); g.summary(a.interval)
                for s in range(T):
                    g.step_intervals(float(t[s]), float(y[s]), bool(has[s]), a.interval)
                return (time.perf_counter() - w0,)

            fns = [("call", call), ("loop", loop), ("filter", ll_filter), ("steps", steps), ("stream", stream)]
            got = {k: [] for k, _ in fns}
            for rep in range(a.warmup + a.repeats):
                for k, fn in fns:                          # alternating: one of each per repeat
                    r = fn()
                    if rep >= a.warmup:
                        got[k].append(r)
            g.run(t, y, has)
            cloud = g.particles()
        rows = T + 1
        _, _, rounds, _ = twin_constants(n)
        key_reads = max(twin_select(cloud[k], a.interval)[1][1] for k in range(d))
        reads = 1 + key_reads
        row_bytes = n * (8 * d + 4) + 8 * (d + 1) * n * (1 + key_reads)
        line = {"probe": "filter_intervals", "model": "c2", "d": d, "n": n, "T": T, "interval": a.interval, "repeats": a.repeats,
                "call_wall_ms": stats([r[0] for r in got["call"]], 1e3), "call_device_ms": stats([r[1] for r in got["call"]]),
                "call_summaries_device_ms": stats([r[2] for r in got["call"]]),
                "loop_wall_ms": stats([r[0] for r in got["loop"]], 1e3), "filter_wall_ms": stats([r[0] for r in got["filter"]], 1e3),
                "steps_wall_ms": stats([r[0] for r in got["steps"]], 1e3), "stream_wall_ms": stats([r[0] for r in got["stream"]], 1e3),
                "launches_per_row_counted": 1 + rounds + 1, "launches_per_row_before": 19,
                "reads_per_row_counted": reads, "reads_per_row_before": 9, "row_bytes_counted": row_bytes,
                "copy_ceiling_gbps": round(gbps.value, 1)}
        cw, lw, sp = line["call_wall_ms"]["median"], line["loop_wall_ms"]["median"], line["loop_wall_ms"]["spread_rel"]
        line["speedup_vs_loop_wall"] = round(lw / cw, 3)
        line["call_below_loop_by_more_than_its_spread"] = bool(cw < lw * (1.0 - sp))
        line["row_wall_us_call_minus_filter"] = round((cw - line["filter_wall_ms"]["median"]) * 1e3 / rows, 3)
        line["row_device_us"] = round(line["call_summaries_device_ms"]["median"] * 1e3 / rows, 3)
        line["row_wall_us_loop_minus_steps"] = round((lw - line["steps_wall_ms"]["median"]) * 1e3 / rows, 3)
        line["row_share_of_copy_ceiling"] = round(row_bytes / (line["row_device_us"] * 1e-6) / 1e9 / gbps.value, 4) if line["row_device_us"] > 0 else None
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
