#!/usr/bin/env python3
"""fleet_smooth_probe.py -- the fleet's backward-simulation smoother (cssm_fleet_smooth, an EXTENSION: forward filtering, backward
simulation of every series in three launches) measured, and set beside cssm_fleet_interpolate on the same fleet, build and GPU.  One
JSON line per shape; the protocol of fleet_interpolate_probe.py.

Shapes: model C2 (d = 3), N particles and n_traj = N trajectories, S series, T records per series of which a block of --gap (a
fraction) carries no observation.  Measured per shape: wall time around the call -- the records of all S x T observations built on the
host included, it ends in the stream's synchronise -- and the device time of its launches (cssm_fleet_smooth_last_ms: forward,
backward simulation, row summaries), median of --repeats calls after --warmup calls of the same shape with their minimum and maximum,
Python's collector off.  The ragged arrays are packed once outside the timed window.

Derived: picoseconds of the backward launch per (trajectory, slot, record) -- S x T x n_traj x N evaluations of the backward kernel --
and what that is in fp64 fused multiply-adds at the vector peak (--peak-tflops, default 78.6: the public FP64 vector figure of the
MI355X; an FMA counts two).  `nominal_ops` is a source-level count of the fp64 operations of one evaluation (two passes of d x (mean,
subtract, divide ~ 10, square-add) plus one exp ~ 30 and the fixed-point digits ~ 10), so `peak_fraction` is an estimate, not a counter.

Against: cssm_fleet_interpolate on the same fleet (it does less work: no backward kernel; the ratio is reported, nothing is gated on
it), and the sequential twin (tests/cpp/backsim_twin.c) on one host core over --twin-T records of one series, as a baseline only."""
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
from composablestatespacemodels_amd import _abi  # noqa: E402
from composablestatespacemodels_amd.filter import FilterFleet, NativePfFleet  # noqa: E402
from fleet_probe import models_of, timed  # noqa: E402


def twin_ps(model, n, T):
    """picoseconds per (trajectory, slot, record) of the twin on one host core: n trajectories over an oracle history of T records"""
    from test_fleet_smooth_host import kinds_of, oracle_history, pack_records, twin_traj
    t, y, has = cases.poisson_counts(T, seed=cases.SEED)
    t = t + 0.5 * np.arange(T)
    _, X, Anc = oracle_history(model, n, cases.SEED, (t, y, has))
    recs, kinds = pack_records(model, n, cases.SEED, t, y, has), kinds_of(model)
    t0 = time.perf_counter()
    twin_traj(X, Anc, recs, kinds, cases.SEED, n)
    return (time.perf_counter() - t0) / ((T - 1) * n * n) * 1e12      # (record 0 has dt = 0: the genealogy, no evaluation)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="c2")
    ap.add_argument("--n", default="100,1000,4096")
    ap.add_argument("--series", default="1024")
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--gap", type=float, default=0.2, help="fraction of the records, in one block, without an observation")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--l2", action="store_true", help="CSSM_OPT_SMOOTH_STAGING = 1: never stage the gathered cloud in LDS")
    ap.add_argument("--peak-tflops", type=float, default=78.6)
    ap.add_argument("--twin-T", type=int, default=3, help="records of the host twin's series; 0: no twin")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    T = a.T
    g0, g1 = T // 3, T // 3 + int(round(a.gap * T))
    lines = []
    gc.disable()
    for name in a.models.split(","):
        for n in (int(x) for x in a.n.split(",")):
            for S in (int(x) for x in a.series.split(",")):
                ms = models_of(name, S)
                d = ms[0].dimension
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
                    fl.set_option(_abi.CSSM_OPT_SMOOTH_STAGING, 1 if a.l2 else 0)
                    off, tt, yy, hh = fl.pack(datas)

                    def smooth():
                        _, _, rc = fl.smooth_packed(off, tt, yy, hh)
                        assert not rc.any()
                        return fl.smooth_last_ms()

                    def interp():
                        _, _, rc = fl.interpolate_packed(off, tt, yy, hh)
                        assert not rc.any()
                        return fl.interpolate_last_ms()
                    rs = timed(smooth, a.repeats, a.warmup)
                    ri = timed(interp, a.repeats, a.warmup)
                med = lambda v: statistics.median(v)
                wall, iwall = med([w for w, _ in rs]), med([w for w, _ in ri])
                fwd, back, rows = (med([m[q] for _, m in rs]) for q in range(3))
                idev = med([m[0] + m[1] for _, m in ri])
                evals = float(S) * (T - 1) * n * n                               # (record 0 of every series has dt = 0)
                ps = back * 1e-3 / evals * 1e12
                nominal = 2 * d * 13 + 40
                line = {"probe": "fleet_smooth", "model": name, "d": d, "n": n, "n_traj": n, "T": T, "gap": [g0, g1], "S": S, "l2": bool(a.l2),
                        "repeats": a.repeats, "wall_ms": round(wall * 1e3, 3), "wall_min_ms": round(min(w for w, _ in rs) * 1e3, 3),
                        "wall_max_ms": round(max(w for w, _ in rs) * 1e3, 3), "forward_ms": round(fwd, 3), "backward_ms": round(back, 3),
                        "backward_min_ms": round(min(m[1] for _, m in rs), 3), "backward_max_ms": round(max(m[1] for _, m in rs), 3),
                        "rows_ms": round(rows, 3), "device_ms": round(fwd + back + rows, 3),
                        "ps_per_traj_slot_record": round(ps, 3), "fma_slots_per_eval_at_peak": round(ps * 1e-12 * a.peak_tflops * 1e12 / 2.0, 2),
                        "nominal_ops": nominal, "peak_fraction": round(nominal / (ps * 1e-12 * a.peak_tflops * 1e12 / 2.0), 4),
                        "interpolate_wall_ms": round(iwall * 1e3, 3), "interpolate_device_ms": round(idev, 3),
                        "wall_ratio_to_interpolate": round(wall / iwall, 2), "device_ratio_to_interpolate": round((fwd + back + rows) / idev, 2)}
                if a.twin_T > 1:
                    line["twin_one_core_ps"] = round(twin_ps(ms[0], n, a.twin_T), 1)
                    line["twin_over_device"] = round(line["twin_one_core_ps"] / ps, 1)
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
