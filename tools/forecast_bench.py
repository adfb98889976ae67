#!/usr/bin/env python3
"""forecast_bench.py -- one JSON line for a multi-horizon forecast (cssm_pf_forecast) of the C2 model (d = 3, Poisson), N = 2^20,
H = 24 horizons, on GPU 0.

Reports the device time of k_forecast and of the selection (HIP events inside the call: cssm_pf_forecast_last_ms; median of the
timed calls), the bytes the two stages move by construction, the on-box copy ceiling (cssm_diag_copy_ceiling) and the fraction of it
each stage reaches, and for scale the rate of the CPU restatement (the oracle's state chain + the host twin of the draws + numpy's
sort, one thread) at N = 2^16.

Bytes by construction, per particle and horizon: k_forecast writes (d + 2) order keys (8 B each); each of the 8 selection passes
reads them again (8 (d + 2) 8 B) and finds its matches in LDS.  The cloud is read once and the carry is written per chunk."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cases  # noqa: E402
from composablestatespacemodels_amd.filter import NativePf  # noqa: E402


def cpu_rate(model, n, H, key):
    from oracle import oracle
    from test_forecast_draws import build_twin
    with tempfile.TemporaryDirectory() as tmp:
        twin = build_twin(tmp)
        desc = model.descriptor()
        L = desc.leaf_array[0]
        dp = C.POINTER(C.c_double)
        o = oracle.OraclePf(desc, n, cases.SEED)
        o.init(0.0)
        t0 = time.perf_counter()
        for h in range(H):
            o.propagate_only(1.0 + h, None, False)
            x = o.proposed()
            o.set_particles(x)
            e = o.eta()
            out = np.zeros(n)
            twin.twin_obs_draw(desc.desc.obs_kind, e.ctypes.data_as(dp), n, L.has_scale, L.scale, desc.desc.obs_df, key, h,
                               out.ctypes.data_as(dp))
            for row in list(x) + [e, out]:
                np.sort(row)
        dt = time.perf_counter() - t0
    return n * H / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=1 << 20)
    ap.add_argument("--horizons", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu-particles", type=int, default=1 << 16)
    a = ap.parse_args()
    model = cases.c2_model()
    n, H = a.particles, a.horizons
    g = NativePf(model, n, cases.SEED)
    t, y, has = cases.poisson_counts(8)
    g.run(t, y, has)
    times = float(t[-1]) + np.arange(1, H + 1, dtype=np.float64)
    key = g.forecast_key()
    g.forecast(times, key)                      # warm-up (first launch of every kernel)
    kern, sel, wall = [], [], []
    for _ in range(a.repeats):
        w0 = time.perf_counter()
        r = g.forecast(times, key)
        wall.append((time.perf_counter() - w0) * 1e3)
        k_ms, s_ms = g.forecast_last_ms()
        kern.append(k_ms); sel.append(s_ms)
    d = g.d
    rows = d + 2
    bytes_kernel = n * d * 8 + n * H * rows * 8
    bytes_select = 8 * n * H * rows * 8
    copy = C.c_double()
    ceiling = None
    if g.lib.cssm_diag_copy_ceiling(0, 1 << 30, 10, C.byref(copy)) == 0:
        ceiling = copy.value
    km, sm = statistics.median(kern), statistics.median(sel)
    line = {
        "workload": f"forecast c2 d={d} N={n} H={H} (cssm_pf_forecast)",
        "device_ms_total": round(km + sm, 4),
        "k_forecast_ms": round(km, 4),
        "selection_ms": round(sm, 4),
        "wall_ms_median": round(statistics.median(wall), 4),
        "gate_ms": 5.0,
        "within_gate": (km + sm) <= 5.0,
        "bytes_k_forecast": bytes_kernel,
        "bytes_selection": bytes_select,
        "gbps_k_forecast": round(bytes_kernel / km / 1e6, 1),
        "gbps_selection": round(bytes_select / sm / 1e6, 1),
        "copy_ceiling_gbps": None if ceiling is None else round(ceiling, 1),
        "fraction_of_ceiling_k_forecast": None if ceiling is None else round(bytes_kernel / km / 1e6 / ceiling, 3),
        "fraction_of_ceiling_selection": None if ceiling is None else round(bytes_select / sm / 1e6 / ceiling, 3),
        "obs_mean_last": float(r["obs_mean"][-1]),
        "repeats": a.repeats,
    }
    g.close()
    cn = a.cpu_particles
    rate = cpu_rate(model, cn, H, key)
    line["cpu_restatement"] = {"particles": cn, "horizons": H, "particle_horizons_per_s": round(rate, 1),
                               "gpu_particle_horizons_per_s": round(n * H / ((km + sm) / 1e3), 1)}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
