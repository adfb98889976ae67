#!/usr/bin/env python3
"""fleet_smc2_probe.py -- cssm_fleet_copy_series and the SMC2 driver over it (composablestatespacemodels_amd/smc2.py), measured.  The
sibling of fleet_more_probe.py, whose protocol this is.  ONE JSON line: {"probe": "fleet_smc2", "copy": {...}, "smc2": {...}}.

(a) copy: model C2 (d = 3), S series of N particles left by one ll_filter of a few records, then per repeat, on ONE fleet:
  * the host route FIRST -- what the library offered before the call: ``particles(k)`` of every series (S launches, S read-backs), then ONE
    ``init_from`` with M = N rows per series and identity picks under the rotation.  Wall time.  It resets ll, clock and observation
    index, which the copy carries: the comparison is of the clouds alone, and the probe asserts them equal;
  * the call SECOND -- ``copy_series`` under the same rotation (every series is source and destination; in lockstep every cloud moves
    twice, into the destination's non-live half and then home): wall time and device time (cssm_fleet_last_ms()[0]), and the bytes the two
    launches move by construction over that device time, next to cssm_diag_copy_ceiling on the same box.
  Median, min and max of --repeats repeats after --warmup of each; the host route's spread, (max - min) / median of its wall time, is
  reported, and the call beats it when its median wall is below the route's by more than that spread:
  call_below_host_route_by_more_than_its_spread.  A difference inside it shows nothing.

(b) smc2: ONE run of SMC2 over FleetEngine on T observations, its wall time split by engine method (steps, clones, proposal filters,
  adoptions, reseeds -- the rest is the driver's numpy and the descriptors of the proposals) and the number of rejuvenations.  One run, no spread:
  stated as such.  gc is off across the timed legs."""
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
from composablestatespacemodels_amd import SMC2, FleetEngine, TimedObservation  # noqa: E402
from composablestatespacemodels_amd.filter import FilterFleet, NativePfFleet  # noqa: E402
from fleet_more_probe import stats  # noqa: E402
from fleet_probe import models_of  # noqa: E402


def copy_leg(n, S, repeats, warmup):
    ms = models_of("c2", S)
    seeds = FilterFleet.keys(cases.SEED, S)
    data = cases.poisson_counts(5, seed=cases.SEED)
    rot = [(k + 1) % S for k in range(S)]
    ident = np.ascontiguousarray(np.broadcast_to(np.arange(n, dtype=np.uint32), (S, n)))
    with NativePfFleet(ms[0], n, S) as fl:
        d = fl.d
        fl.set_params(ms); fl.reseed(seeds)

        def start():
            rc = fl.ll_filter([data] * S)[3]
            assert not rc.any()

        def host_route():
            t0 = time.perf_counter()
            clouds = [fl.particles(k) for k in range(S)]
            _, rc = fl.init_from(float(data[0][-1]), [clouds[j].T for j in rot], picks=ident)
            w = time.perf_counter() - t0
            assert not rc.any()
            return w, clouds

        def call():
            t0 = time.perf_counter()
            rc = fl.copy_series(rot)
            w = time.perf_counter() - t0
            assert not rc.any()
            return w, fl.last_ms()[0]

        route, calls = [], []
        for rep in range(warmup + repeats):
            start(); w_route, clouds = host_route()
            start(); w_call, dev = call()
            if rep >= warmup:
                route.append(w_route); calls.append((w_call, dev))
        for k in (0, 1, S - 1):                                  # the same clouds, whichever way they came
            assert np.array_equal(fl.particles(k), clouds[rot[k]])
        ceiling = C.c_double(0.0)
        have = fl.lib.cssm_diag_copy_ceiling(0, 1 << 30, 10, C.byref(ceiling)) == 0
    per_series = d * n * 8 + n * 4 + 32                          # cloud, ancestors, scalars
    moved = 2 * S * per_series + 2 * S * per_series              # read + written, by either launch (lockstep: every cloud settles)
    e = {"model": "c2", "d": d, "n": n, "S": S, "repeats": repeats, "map": "rotation by one",
         "host_route_wall_ms": stats(route, 1e3), "wall_ms": stats([w for w, _ in calls], 1e3), "device_ms": stats([v for _, v in calls]),
         "bytes_moved": moved}
    dev = e["device_ms"]["median"]
    e["device_gb_per_s"] = round(moved / (dev * 1e-3) / 1e9, 1) if dev > 0 else None
    e["copy_ceiling_gb_per_s"] = round(ceiling.value, 1) if have else None
    e["fraction_of_ceiling"] = round(e["device_gb_per_s"] / ceiling.value, 3) if have and dev > 0 and ceiling.value > 0 else None
    hw, sp = e["host_route_wall_ms"]["median"], e["host_route_wall_ms"]["spread_rel"]
    e["speedup_vs_host_route_wall"] = round(hw / e["wall_ms"]["median"], 1)
    e["call_below_host_route_by_more_than_its_spread"] = bool(e["wall_ms"]["median"] < hw * (1.0 - sp))
    return e


class TimedEngine(FleetEngine):
    """FleetEngine with the wall time of every method summed (each ends in a stream synchronise)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.wall = {"step": 0.0, "clone": 0.0, "propose": 0.0, "adopt": 0.0, "reseed": 0.0}
        self.count = {k: 0 for k in self.wall}

    def _timed(self, name, fn, *a):
        t0 = time.perf_counter()
        out = fn(*a)
        self.wall[name] += time.perf_counter() - t0
        self.count[name] += 1
        return out

    def step(self, *a):
        return self._timed("step", super().step, *a)

    def clone(self, *a):
        return self._timed("clone", super().clone, *a)

    def propose(self, *a):
        return self._timed("propose", super().propose, *a)

    def adopt(self, *a):
        return self._timed("adopt", super().adopt, *a)

    def reseed(self, *a):
        return self._timed("reseed", super().reseed, *a)


def smc2_leg(n, S, T, spread):
    base = np.asarray(cases.c2_params().flattenParams())
    rng = np.random.default_rng(cases.SEED)
    draws = [cases.c2_params().withFlat(base + spread * rng.standard_normal(base.size)) for _ in range(S)]

    def log_prior(th):
        z = (np.asarray(th) - base) / spread
        return float(-0.5 * np.sum(z * z))

    t, y, has = cases.poisson_counts(T, seed=cases.SEED)
    obs = [TimedObservation(float(a), float(b) if h else None) for a, b, h in zip(t, y, has)]
    eng = TimedEngine(cases.c2_model(), n, S)
    with SMC2(cases.c2_unparam(), draws, n, log_prior=log_prior, seed=cases.SEED, engine=eng) as smc:
        t0 = time.perf_counter()
        states = smc.run(obs)
        wall = time.perf_counter() - t0
        e = {"model": "c2", "d": 3, "n": n, "S": S, "T": T, "prior_sd": spread, "runs": 1, "wall_s": round(wall, 3),
             "rejuvenations": smc.rejuvenations, "accepted": int(sum(s.accepted for s in states)),
             "log_evidence": states[-1].log_evidence, "final_ess": round(states[-1].ess, 1)}
    for k, v in eng.wall.items():
        e[k + "_s"] = round(v, 3)
        e[k + "_calls"] = eng.count[k]
    e["driver_s"] = round(wall - sum(eng.wall.values()), 3)
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--series", type=int, default=1024)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--prior-sd", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--skip-smc2", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    gc.disable()
    out = {"probe": "fleet_smc2", "copy": copy_leg(a.n, a.series, a.repeats, a.warmup)}
    if not a.skip_smc2:
        out["smc2"] = smc2_leg(a.n, a.series, a.T, a.prior_sd)
    gc.enable()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
