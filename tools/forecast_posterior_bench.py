#!/usr/bin/env python3
"""forecast_posterior_bench.py -- one JSON line for a forecast from a joint posterior sample (cssm_pf_forecast_posterior) of the C2
model (d = 3, Poisson), N = 2^20 particles, H = 24 horizons, M = 10^4 distinct parameter sets, on GPU 0, beside the same-process
single-parameter forecast (cssm_pf_forecast) of the same handle, times and key.

Device times are HIP events inside the calls (cssm_pf_forecast_last_ms; median of the timed calls).  Bytes by construction, per
particle and horizon, as tools/forecast_bench.py counts them, plus the posterior's inputs: k_forecast_post gathers a state row
(d doubles) once and a parameter row (3 d + 1 doubles) once per chunk, from tables of M rows that stay in L2."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cases  # noqa: E402
from composablestatespacemodels_amd.filter import NativePf  # noqa: E402


def timed(g, call, repeats):
    call()                                      # warm-up (first launch of every kernel)
    kern, sel = [], []
    for _ in range(repeats):
        r = call()
        k_ms, s_ms = g.forecast_last_ms()
        kern.append(k_ms); sel.append(s_ms)
    return statistics.median(kern), statistics.median(sel), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=1 << 20)
    ap.add_argument("--horizons", type=int, default=24)
    ap.add_argument("--pairs", type=int, default=10_000)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    model = cases.c2_model()
    n, H, M = a.particles, a.horizons, a.pairs
    g = NativePf(model, n, cases.SEED)
    t, y, has = cases.poisson_counts(8)
    g.run(t, y, has)
    t0 = float(t[-1])
    times = t0 + np.arange(1, H + 1, dtype=np.float64)
    key = g.forecast_key()
    rng = np.random.default_rng(cases.SEED)
    th0 = np.asarray(model.parameters().flattenParams())
    theta = th0 + 0.1 * rng.standard_normal((M, th0.size))
    d = g.d
    x = 0.5 * rng.standard_normal((M, d))
    pk, ps, rp = timed(g, lambda: g.forecast_posterior(theta, x, t0, times, key), a.repeats)
    fk, fs, _ = timed(g, lambda: g.forecast(times, key), a.repeats)
    rows = d + 2
    bytes_kernel = n * H * rows * 8 + n * (d + 3 * d + 1) * 8
    line = {
        "workload": f"forecast_posterior c2 d={d} N={n} H={H} M={M} (cssm_pf_forecast_posterior)",
        "device_ms_total": round(pk + ps, 4),
        "k_forecast_post_ms": round(pk, 4),
        "selection_ms": round(ps, 4),
        "forecast_device_ms_total": round(fk + fs, 4),
        "k_forecast_ms": round(fk, 4),
        "forecast_selection_ms": round(fs, 4),
        "ratio_to_forecast": round((pk + ps) / (fk + fs), 3),
        "target_ratio": 1.5,
        "within_target": (pk + ps) <= 1.5 * (fk + fs),
        "bytes_k_forecast_post": bytes_kernel,
        "gbps_k_forecast_post": round(bytes_kernel / pk / 1e6, 1),
        "distinct_pairs_taken": int(np.unique(rp["pick"]).size),
        "obs_mean_last": float(rp["obs_mean"][-1]),
        "repeats": a.repeats,
    }
    g.close()
    print(json.dumps(line))


if __name__ == "__main__":
    main()
