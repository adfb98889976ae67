#!/usr/bin/env python3
"""smooth_probe.py -- the single handle's backward-simulation smoother (cssm_pf_smooth, an EXTENSION: cssm_pf_interpolate's forward pass,
then backward simulation with the slots of the cloud tiled over many workgroups) measured, and set beside cssm_pf_interpolate on the same
handle, build and GPU, and -- where a fleet holds the cloud -- beside cssm_fleet_smooth of a one-series fleet.  One JSON line per shape;
the protocol of fleet_smooth_probe.py.

Shapes: model C2 (d = 3), --shapes N:n_traj pairs, T records of which a block of --gap (a fraction) carries no observation.  Measured
per shape: wall time around the call (the records built on the host included; it ends in the stream's synchronise) and the device time
of its launches (cssm_pf_smooth_last_ms: forward, backward simulation, row summaries), median of --repeats calls after --warmup calls
of the same shape with their minimum and maximum, Python's collector off.

Derived: picoseconds of the backward launches per (trajectory, slot, record) -- (T - 1) x n_traj x N evaluations of the backward kernel
(record 0 has dt = 0: the genealogy), each formed twice (the level's pass and the sums' pass) -- the figure fleet_smooth_probe.py reports
for k_fleet_backsim.  --tile sets CSSM_OPT_SMOOTH_TILE."""
from __future__ import annotations

import argparse
import gc
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import cases  # noqa: E402
from composablestatespacemodels_amd import _abi  # noqa: E402
from composablestatespacemodels_amd.filter import NativePf, NativePfFleet  # noqa: E402
from fleet_probe import timed  # noqa: E402


def spread(values, digits=3):
    return {"median": round(statistics.median(values), digits), "min": round(min(values), digits), "max": round(max(values), digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096:4096,65536:1000,1048576:1000", help="N:n_traj pairs")
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--gap", type=float, default=0.2, help="fraction of the records, in one block, without an observation")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tile", type=int, default=0, help="CSSM_OPT_SMOOTH_TILE (0: the default)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    T = a.T
    g0, g1 = T // 3, T // 3 + int(round(a.gap * T))
    t, y, has = cases.poisson_counts(T, seed=cases.SEED)
    has = has.copy(); has[g0:g1] = 0
    model = cases.c2_model()
    lines = []
    gc.disable()
    for shape in a.shapes.split(","):
        n, M = (int(x) for x in shape.split(":"))
        with NativePf(model, n, cases.SEED) as g:
            g.set_option(_abi.CSSM_OPT_SMOOTH_TILE, a.tile)

            def smooth():
                g.smooth(t, y, has, n_traj=M)
                return g.smooth_last_ms()

            def interp():
                g.interpolate(t, y, has)
                return None
            rs = timed(smooth, a.repeats, a.warmup)
            ri = timed(interp, a.repeats, a.warmup)
        evals = float(T - 1) * M * n
        back = [m[1] for _, m in rs]
        line = {"probe": "smooth", "model": "c2", "d": 3, "n": n, "n_traj": M, "T": T, "gap": [g0, g1], "tile": a.tile or _abi.SMOOTH_TILE,
                "repeats": a.repeats, "wall_ms": spread([w * 1e3 for w, _ in rs]), "forward_ms": spread([m[0] for _, m in rs]),
                "backward_ms": spread(back), "rows_ms": spread([m[2] for _, m in rs]),
                "ps_per_traj_slot_record": spread([b * 1e-3 / evals * 1e12 for b in back]),
                "interpolate_wall_ms": spread([w * 1e3 for w, _ in ri])}
        if n <= _abi.FLEET_MAX_N:
            with NativePfFleet(model, n, 1) as fl:
                fl.reseed([cases.SEED])
                off, tt, yy, hh = fl.pack([(t, y, has)])

                def fleet():
                    _, _, rc = fl.smooth_packed(off, tt, yy, hh, n_traj=M)
                    assert not rc.any()
                    return fl.smooth_last_ms()
                rf = timed(fleet, a.repeats, a.warmup)
            fb = [m[1] for _, m in rf]
            line["fleet_wall_ms"] = spread([w * 1e3 for w, _ in rf])
            line["fleet_backward_ms"] = spread(fb)
            line["fleet_ps_per_traj_slot_record"] = spread([b * 1e-3 / evals * 1e12 for b in fb])
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
