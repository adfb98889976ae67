#!/usr/bin/env python3
"""fleet_pmmh_probe.py -- PMMH on a fleet (cssm_fleet_pmmh_run: a chain per series, one launch per iteration) against the batch of
chains (cssm_pmmh_run_batched: 64 chains, each spread over the GPU, two launches per observation), in the same process on the same
GPU.  One JSON line per shape.

Shapes: model C2 (d = 3), N particles, T observations, S chains, chain k on its own data, start and seed.
Measured per shape, protocol of tools/fleet_probe.py (median of --repeats calls after --warmup calls of the same shape, Python's
collector off, arrays packed outside the timed window):
  * wall time around cssm_fleet_pmmh_run of --iters iterations -> iterations per second per chain and in total (chain-iterations);
  * the split of an iteration (cssm_fleet_pmmh_last_split): propose + set_params + reseed, record building, upload, kernel, decide;
  * cssm_fleet_filter with last_out only against cssm_fleet_ll_filter on the same fleet and data: wall and cssm_fleet_last_ms.
Baseline: cssm_pmmh_run_batched with 64 chains at the same N and T (shared data: the batch has no other shape), --spread times, scaled
by S / 64 (exact for ceil(S / 64) batches one after the other); its spread is the margin the factor has to clear."""
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
from composablestatespacemodels_amd.filter import NativePfFleet  # noqa: E402
from fleet_probe import perturbed, timed  # noqa: E402

DP, U64, U8, I32 = C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="100,1000")
    ap.add_argument("--series", default="64,1024,4096")
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--iters", type=int, default=2, help="iterations per timed call")
    ap.add_argument("--delta", type=float, default=0.05)
    ap.add_argument("--repeats", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--spread", type=int, default=5, help="repeats of the baseline")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    T, iters = a.T, a.iters
    lib = _abi.load_library()
    um = cases.c2_unparam()
    seven = [perturbed(cases.c2_params, k) for k in range(7)]
    model = um.run(seven[0])
    desc = model.descriptor()
    nt = len(seven[0].flattenParams())
    d = model.dimension
    lines = []
    gc.disable()
    for n in (int(x) for x in a.n.split(",")):
        # the baseline: 64 chains in one batch, shared data
        t0, y0, h0 = cases.poisson_counts(T, seed=cases.SEED)
        h0 = np.ascontiguousarray(h0, dtype=np.uint8)
        th64 = np.ascontiguousarray([seven[k % 7].flattenParams() for k in range(64)], dtype=np.float64)
        sd64 = np.arange(64, dtype=np.uint64) + np.uint64(cases.SEED + 100)
        o64 = (np.zeros((64, iters)), np.zeros((64, iters, nt)), np.zeros((64, iters), dtype=np.int32), np.zeros((64, iters, d)))
        hb = C.c_void_p()
        _abi.check(lib.cssm_pfb_create(desc.ptr(), n, 64, 0, C.byref(hb)))

        def batched():
            _abi.check(lib.cssm_pmmh_run_batched(hb, desc.ptr(), th64.ctypes.data_as(DP), nt, a.delta, t0.ctypes.data_as(DP), y0.ctypes.data_as(DP),
                                                 h0.ctypes.data_as(U8), T, sd64.ctypes.data_as(U64), iters, o64[0].ctypes.data_as(DP),
                                                 o64[1].ctypes.data_as(DP), o64[2].ctypes.data_as(I32), o64[3].ctypes.data_as(DP)))
        tb = [w for w, _ in timed(batched, a.spread, 1)]
        lib.cssm_pfb_destroy(hb)
        b_med = statistics.median(tb)
        for S in (int(x) for x in a.series.split(",")):
            packed = NativePfFleet.pack([cases.poisson_counts(T, seed=cases.SEED + k) for k in range(S)])
            off, t, y, has = packed
            th0 = np.ascontiguousarray([seven[k % 7].flattenParams() for k in range(S)], dtype=np.float64)
            sd = np.arange(S, dtype=np.uint64) + np.uint64(cases.SEED + 100)
            out = (np.zeros((S, iters)), np.zeros((S, iters, nt)), np.zeros((S, iters), dtype=np.int32), np.zeros((S, iters, d)))
            with NativePfFleet(model, n, S) as fl:
                def run():
                    _abi.check(lib.cssm_fleet_pmmh_run(fl._h, desc.ptr(), th0.ctypes.data_as(DP), nt, a.delta, off.ctypes.data_as(U64), t.ctypes.data_as(DP),
                                                       y.ctypes.data_as(DP), has.ctypes.data_as(U8), sd.ctypes.data_as(U64), iters, out[0].ctypes.data_as(DP),
                                                       out[1].ctypes.data_as(DP), out[2].ctypes.data_as(I32), out[3].ctypes.data_as(DP)))
                    return fl.pmmh_last_split()[0]
                r = timed(run, a.repeats, a.warmup)
                # the fleet is left under the last iteration's proposals: filter with the last rows only against ll_filter, as it stands

                def last_only():
                    rc = fl.filter_packed(*packed, want_path=False)[5]
                    assert set(int(v) for v in rc) <= {0, _abi.CSSM_ENONFINITE}
                    return fl.last_ms()[0]

                def plain():
                    rc = fl.ll_filter_packed(*packed)[3]
                    assert set(int(v) for v in rc) <= {0, _abi.CSSM_ENONFINITE}
                    return fl.last_ms()[0]
                rl = timed(last_only, a.repeats, a.warmup)
                rp = timed(plain, a.repeats, a.warmup)
            wall = statistics.median(w for w, _ in r)
            split = [statistics.median(s[q] for _, s in r) / iters for q in range(5)]
            it_s_chain = iters / wall
            b_scaled = b_med * S / 64
            med = lambda v: statistics.median(v)
            line = {"probe": "fleet_pmmh", "model": "c2", "d": d, "n": n, "T": T, "S": S, "iters_per_call": iters, "repeats": a.repeats,
                    "wall_ms_per_iteration": round(wall / iters * 1e3, 4), "iterations_per_s_per_chain": round(it_s_chain, 3),
                    "chain_iterations_per_s": round(it_s_chain * S, 1),
                    "wall_min_ms": round(min(w for w, _ in r) / iters * 1e3, 4), "wall_max_ms": round(max(w for w, _ in r) / iters * 1e3, 4),
                    "split_ms_per_iteration": {k: round(v, 4) for k, v in zip(("propose_set_params", "build_records", "upload", "kernel", "decide"), split)},
                    "batched_ms_per_iteration_64": [round(x / iters * 1e3, 3) for x in tb],
                    "batched_spread_rel": round((max(tb) - min(tb)) / b_med, 4),
                    "batched_chain_iterations_per_s": round(64 * iters / b_med, 1),
                    "batched_scaled_ms_per_iteration": round(b_scaled / iters * 1e3, 3),
                    "factor_vs_batched": round(b_scaled / wall, 3),
                    "filter_last_only_wall_ms": round(med([w for w, _ in rl]) * 1e3, 4), "filter_last_only_device_ms": round(med([v for _, v in rl]), 4),
                    "ll_filter_wall_ms": round(med([w for w, _ in rp]) * 1e3, 4), "ll_filter_device_ms": round(med([v for _, v in rp]), 4)}
            line["last_only_over_ll_filter_wall"] = round(line["filter_last_only_wall_ms"] / line["ll_filter_wall_ms"], 4)
            line["last_only_over_ll_filter_device"] = round(line["filter_last_only_device_ms"] / line["ll_filter_device_ms"], 4)
            print(json.dumps(line), flush=True)
            lines.append(line)
    gc.enable()
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
