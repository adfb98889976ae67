#!/usr/bin/env python3
"""Walk the single handle's drivers over the shapes at which a launch decision flips, T = 3 records each, so that a kernel trace of
the run lists every launch the host code decides on:

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python3 tools/launch_trace.py
    python3 tools/launch_trace.py --list OUT      # the ordered (kernel, grid, workgroup) lines of that trace, their count and hash

Two builds of the library (CSSM_PF_LIB picks one) that take the same decisions give the same list line for line.  step, run, run_more,
run(want_path), filter_intervals and interpolate on every handle, the options that steer the plan at 2^20 particles, a 2-chain batch, and
a series with an outlying observation through every driver (the hold and its redo)."""
import csv
import glob
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def listing(out_dir):
    rows = []
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            g = lambda stem: tuple(int(r[f"{stem}_{a}"]) for a in "XYZ")
            rows.append((int(r["Start_Timestamp"]), r["Kernel_Name"], g("Grid_Size"), g("Workgroup_Size")))
    rows.sort()
    lines = [f"{name} {grid} {wg}" for _, name, grid, wg in rows]
    return lines, hashlib.sha256("\n".join(lines).encode()).hexdigest()


def drivers(g, t, y, has, interp=True):
    g.init(0.0)
    for s in range(len(t)):
        g.step(t[s], y[s], bool(has[s]))
    g.run(t, y, has)
    g.run_more(t + t[-1] + 1.0, y, has)
    g.run(t, y, has, want_path=True)
    g.filter_intervals(t, y, has)
    if interp:
        g.interpolate(t, y, has)


def main():
    import numpy as np
    import cases
    from composablestatespacemodels_amd.filter import NativePf, NativePfBatch

    models = (cases.c1_model(), cases.c2_model(), cases.dim_model(9))
    t, y, has = cases.poisson_counts(3)
    has = has.copy(); has[1] = 0
    for model in models:
        for n in (1000, 100000, (1 << 20) - 1024, 1 << 20, (1 << 20) + 1, 1 << 21, (1 << 22) + 1024):
            g = NativePf(model, n, cases.SEED)
            drivers(g, t, y, has, interp=n <= 1 << 21)
            g.close()
        for option, values in ((3, (0,)), (2, (1, 2)), (6, (1, 2, 3)), (7, (0,)), (10, (0, 2))):   # fused sums, resampler, whole tiles, group sums, wave sums
            for v in values:
                g = NativePf(model, 1 << 20, cases.SEED)
                g.set_option(option, v)
                drivers(g, t, y, has, interp=False)
                g.close()
    b = NativePfBatch(models[1], 5000, 2)
    b.filter([models[1]] * 2, [cases.SEED, cases.SEED + 1], t, y, has)
    b.filter([models[1]] * 2, [cases.SEED, cases.SEED + 1], t, y, has, want_path=False)
    b.close()
    # an outlying observation per driver: the series is held at it and the observation redone (interpolate: the series run again)
    t, y, has = cases.poisson_counts(10)
    y = y.copy(); y[4] = 60.0; y[9] = 60.0
    has = has.copy(); has[5] = 0
    for fused in (1, 0):
        g = NativePf(models[1], 5000, cases.SEED)
        g.set_option(3, fused)
        drivers(g, t, y, has)
        g.run(t[:4], y[:4], has[:4])
        g.run_more(t[4:], y[4:], has[4:])
        g.close()
    print("launch_trace: done")


if __name__ == "__main__":
    if sys.argv[1:2] == ["--list"]:
        lines, digest = listing(sys.argv[2])
        if len(sys.argv) > 3:
            open(sys.argv[3], "w").write("\n".join(lines) + "\n")
        print(f"{len(lines)} launches, sha256 {digest}")
    else:
        main()
