#!/usr/bin/env python3
"""if2_probe.py -- iterated filtering with one large swarm (cssm_pf_if2, an EXTENSION; the single-handle form of cssm_fleet_if2) measured on
one device.  One JSON line per shape.  Speed is reported, not gated.

Shape: model C2 (d = 3, 10 stored parameters), T = 100 records (a tenth unobserved), 20 iterations; one warm-up call, then the median,
minimum and maximum of --repeats calls, Python's collector off.

  * like for like: cssm_pf_if2 at N = 4096 against a one-series cssm_fleet_if2 at N = 4096 -- same build, the calls alternating, the
    results asserted equal bit for bit.  The only comparison the fleet path offers: it ends at 4096 particles.
  * larger clouds (--n, default 2^16 and 2^20): wall time around the call (the records built on the host, the uploads and the read-back of
    the rows included; it ends in the stream's synchronise), device time of its launches (cssm_pf_if2_last_ms), and device nanoseconds
    per (iteration, record, particle) -- to set beside the 0.113 ns recorded for k_fleet_if2 at S = 1024 x N = 1000.
  * bytes: per particle of a WEIGHTED record, counted from the shapes of what the five launches read and write --
      k_if2_weigh      4 (ancestor) + 8 n_theta (theta gathered) + 8 n_theta (theta written) + 8 d + 8 d (x likewise) + 8 (log-weight)
      k_if2_sums       8 + 8 (the log-weight read, the weight written)
      k_if2_ends       8 (the weight) + 4 (the end slot)
      k_if2_offspring  4 (an end slot; the rest of the search hits lines its neighbours fetched) + 4 (the ancestor)
    = 16 (n_theta + d) + 48; an unweighted record moves the first line less the log-weight plus the identity ancestor.  The particle's
    re-reads of its own fresh theta row (the coefficients) are cache hits and not counted.  The records' bytes over the device time, as a
    share of cssm_diag_copy_ceiling on the same device; the start and end launches of an iteration (3 of 3 + 4.6 T launches) are in the
    time and not in the bytes.
  * launches per record (5 weighted, 1 unweighted; 3 more per iteration) and the host's share, wall minus device."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import cases  # noqa: E402
from composablestatespacemodels_amd import _abi  # noqa: E402
from composablestatespacemodels_amd.filter import NativePf, NativePfFleet  # noqa: E402
from fleet_probe import timed  # noqa: E402


def spread(rs, idx, scale):
    v = [r[idx] * scale if idx == 0 else r[1][idx - 1] * scale for r in rs]
    return round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="65536,1048576")
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rw-sd", type=float, default=0.02)
    ap.add_argument("--cooling", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    model = cases.c2_model()
    th = np.array(model.parameters().flattenParams())
    nt, d = len(th), 3
    sd = np.full(nt, a.rw_sd)
    T, M, seed = a.T, a.iters, cases.SEED
    data = cases.poisson_counts(T, seed=cases.SEED, missing=0.1)
    weighted = int(np.count_nonzero(data[2]))
    launches = M * (3 + 5 * weighted + (T - weighted))
    gbps = C.c_double()
    _abi.check(_abi.load_library().cssm_diag_copy_ceiling(0, 1 << 30, 5, C.byref(gbps)))
    lines = []
    gc.disable()
    # like for like at the fleet's largest cloud: the two calls alternate
    n = _abi.FLEET_MAX_N
    with NativePf(model, n) as pf, NativePfFleet(model, n, 1) as fl:
        got = {}

        def both():
            got["one"] = pf.if2(*data, sd, a.cooling, M, seed, theta0=th, want_swarm=True)
            ms_one = pf.if2_last_ms()
            t0 = time.perf_counter()
            got["fleet"] = fl.if2(model.descriptor(), [data], sd, a.cooling, M, [seed], theta0=th[None], want_swarm=True)
            return ms_one, fl.if2_last_ms(), time.perf_counter() - t0
        rs = timed(both, a.repeats, a.warmup)
        for key in ("theta_mean", "ll", "swarm"):
            np.testing.assert_array_equal(got["one"][key], got["fleet"][key][0])
        fleet_wall = [r[1][2] for r in rs]
        one_wall = [r[0] - r[1][2] for r in rs]
        line = {"probe": "if2_vs_fleet", "model": "c2", "n": n, "T": T, "iters": M, "repeats": a.repeats, "bit_equal": True,
                "single_device_ms": spread(rs, 1, 1.0), "fleet_device_ms": spread(rs, 2, 1.0),
                "single_wall_ms": [round(statistics.median(one_wall) * 1e3, 3), round(min(one_wall) * 1e3, 3), round(max(one_wall) * 1e3, 3)],
                "fleet_wall_ms": [round(statistics.median(fleet_wall) * 1e3, 3), round(min(fleet_wall) * 1e3, 3), round(max(fleet_wall) * 1e3, 3)],
                "single_launches": launches, "fleet_launches": 1}
        print(json.dumps(line), flush=True)
        lines.append(line)
    for n in (int(x) for x in a.n.split(",")):
        with NativePf(model, n) as pf:
            def search():
                out = pf.if2(*data, sd, a.cooling, M, seed, theta0=th)
                assert out["rc"] == 0
                return (pf.if2_last_ms(),)
            rs = timed(search, a.repeats, a.warmup)
        wall, dev = spread(rs, 0, 1e3), spread(rs, 1, 1.0)
        steps = float(M) * T * n
        rec_bytes = float(M) * n * (weighted * (16 * (nt + d) + 48) + (T - weighted) * (16 * (nt + d) + 8))
        line = {"probe": "if2", "model": "c2", "d": d, "n_theta": nt, "n": n, "T": T, "weighted": weighted, "iters": M, "repeats": a.repeats,
                "wall_ms": wall, "device_ms": dev, "host_share_ms": round(wall[0] - dev[0], 3),
                "ns_per_particle_step": round(dev[0] * 1e-3 / steps * 1e9, 4), "fleet_recorded_ns_per_particle_step": 0.113,
                "launches": launches, "launches_per_weighted_record": 5, "launches_per_unweighted_record": 1, "launches_per_iteration": 3,
                "us_per_launch": round(dev[0] * 1e3 / launches, 2),
                "bytes_per_particle_weighted_record": 16 * (nt + d) + 48, "record_gb_per_s": round(rec_bytes / (dev[0] * 1e-3) / 1e9, 1),
                "copy_ceiling_gb_per_s": round(gbps.value, 1), "share_of_copy_ceiling": round(rec_bytes / (dev[0] * 1e-3) / 1e9 / gbps.value, 4)}
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
