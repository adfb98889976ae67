#!/usr/bin/env python3
"""fleet_lgcp_probe.py -- the LGCP fleet (cssm_fleet_create_lgcp: FilterLgcp of S Cox-process event streams in ONE launch, one workgroup
per stream) against what a user had to do before it, in the same process.  One JSON line per shape; the protocol of
fleet_filter_forecasts_probe.py.

Shapes: model C4 at precision 2, N particles, S event streams drawn by simulate_lgcp on [0, 10] (about 12 events per stream; a stream
without an event is left out and counted).  Per repeat, ALTERNATING:
  * the call: cssm_fleet_ll_filter on arrays packed once outside the timed window -- wall time (it ends in the stream's synchronise) and
    device time (cssm_fleet_last_ms()[0]);
  * the loop, which is the parent commit's path: cssm_pf_reseed + cssm_pf_ll_filter per stream on ONE reused handle of the same N, under
    the keys the fleet runs -- timed over the first --loop-series streams and scaled to S by the events they hold.
Median, min and max of --repeats (at least 7) alternations after --warmup of each; the call beats the loop when its median wall is below
the scaled loop's by more than the loop's own spread, (max - min) / median: call_below_loop_by_more_than_its_spread.  Also stated: the
workload's sum of sub-steps (n_sub as the records hold it: cssm_fleet_pack_record_lgcp) and the call's device time per particle and
sub-step -- the launch is bound by arithmetic, so this is its figure of merit."""
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
from composablestatespacemodels_amd.filter import FilterFleet, NativeLgcpFleet, NativePf  # noqa: E402
from composablestatespacemodels_amd.simulate import lgcp_fleet_data, simulate_lgcp  # noqa: E402


def stats(v, scale=1.0, digits=4):
    v = [x * scale for x in v]
    med = statistics.median(v)
    return {"median": round(med, digits), "min": round(min(v), digits), "max": round(max(v), digits),
            "spread_rel": round((max(v) - min(v)) / med, 4) if med > 0 else None}


def sub_steps(lib, desc, times):
    """the sum of n_sub over a stream's records, read from the records themselves"""
    buf, nb, nf = (C.c_uint8 * 1024)(), C.c_size_t(), C.c_size_t()
    total, tp = 0, float(times[0])
    for s, t in enumerate(times):
        rc = lib.cssm_fleet_pack_record_lgcp(desc.ptr(), 1, 0, tp, float(t), s, buf, 1024, C.byref(nb), None, 0, C.byref(nf))
        assert rc == 0
        total += int(np.frombuffer(bytes(buf[16:20]), dtype=np.int32)[0])
        tp = float(t)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="100,1000,4096")
    ap.add_argument("--series", default="1024")
    ap.add_argument("--precision", type=int, default=2)
    ap.add_argument("--end", type=float, default=10.0)
    ap.add_argument("--loop-series", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.repeats < 7:
        ap.error("at least 7 repeats")
    model = cases.c4_model()
    desc = model.descriptor(a.precision)
    lines = []
    gc.disable()
    for n in (int(x) for x in a.n.split(",")):
        for S_asked in (int(x) for x in a.series.split(",")):
            sim = simulate_lgcp(model, 0.0, a.end, a.precision, n_paths=S_asked, keep_grid=False)
            datas = [d for d in lgcp_fleet_data(sim) if len(d)]
            S = len(datas)
            keys = FilterFleet.keys(cases.SEED, S)
            L = min(a.loop_series, S)
            with NativeLgcpFleet(model, n, S, a.precision) as fl, NativePf(model, n, keys[0], lgcp_precision=a.precision) as g:
                fl.reseed(keys)
                off, t, y, has = fl.pack(datas)
                nsub = [sub_steps(fl.lib, desc, d) for d in datas]
                ev = [(np.ascontiguousarray(d), np.ones(len(d)), np.ones(len(d), dtype=np.uint8)) for d in datas[:L]]

                def call():
                    t0 = time.perf_counter()
                    ll, _, _, rc = fl.ll_filter_packed(off, t, y, has)
                    w = time.perf_counter() - t0
                    assert not rc.any()
                    return w, fl.last_ms()[0], ll

                def loop():
                    out = np.zeros(L)
                    t0 = time.perf_counter()
                    for k in range(L):
                        g.reseed(keys[k])
                        out[k] = g.run(*ev[k])[0]
                    return time.perf_counter() - t0, 0.0, out

                fns = [("call", call)] + ([] if a.no_baseline else [("loop", loop)])
                got = {k: [] for k, _ in fns}
                for rep in range(a.warmup + a.repeats):
                    for k, fn in fns:                              # alternating: one of each per repeat
                        r = fn()
                        if rep >= a.warmup:
                            got[k].append(r)
                if not a.no_baseline:                              # the two paths filter the same streams to the same bits
                    assert np.array_equal(got["call"][0][2][:L], got["loop"][0][2])
            R, total = int(off[-1]), int(sum(nsub))
            line = {"probe": "fleet_lgcp", "model": "c4", "d": 1, "precision": a.precision, "n": n, "S": S, "S_empty": S_asked - S, "events": R,
                    "sub_steps": total, "repeats": a.repeats,
                    "wall_ms": stats([w for w, _, _ in got["call"]], 1e3), "device_ms": stats([d for _, d, _ in got["call"]])}
            line["device_ns_per_particle_sub_step"] = round(line["device_ms"]["median"] * 1e6 / (total * n), 5)
            line["wall_us_per_event"] = round(line["wall_ms"]["median"] * 1e3 / R, 4)
            if not a.no_baseline:
                scale = R / float(sum(len(d) for d in datas[:L]))
                line["loop_series"] = L
                line["loop_wall_ms_scaled"] = stats([w * scale for w, _, _ in got["loop"]], 1e3)
                lw, sp = line["loop_wall_ms_scaled"]["median"], line["loop_wall_ms_scaled"]["spread_rel"]
                line["loop_wall_us_per_event"] = round(lw * 1e3 / R, 4)
                line["speedup_vs_loop_wall"] = round(lw / line["wall_ms"]["median"], 3)
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
