#!/usr/bin/env python3
"""Cost of the supernova explosion of the time loop (code_running.py:361-396, the block that changes N) on the two-phase
cube: Simulation.supernova_explosion on the resident state against the host route a user had to take before it existed.

The N-particle two-phase cube, one step; --stars gas rows drawn (seeded) and turned into 20 M_sun stars.

  host route   download and download_composition, compat.supernova_explosion and compat.supernova_insert on the whole
               state, a new Simulation from the result and the step it needs before a phase can run (that step averages
               with a zero old acceleration: not the driver's update, drv:482-485).  Host clock per part.  Only entry
               points older than the resident call, but for the two host functions: on a build without them (an older
               checkout) pass --host-functions PATH, a newer checkout's sph-code_amd/compat.py, from which
               supernova_explosion and supernova_insert are taken (NumPy on the host; no library call).
  resident     (where the library has it) per repeat Simulation.supernova_explosion on a state stepped once: the host
               clock of the call - the rows' download, the host's NumPy on them, the insertion, the search - and the
               device time per stage of the insertion (upload | grow | insert | search), the buffers reallocated.  Every
               repeat starts from a fresh Simulation of the same state, so the repeats do the same work.

Prints one JSON line; --out FILE (meant for profiles/latest_insert_profile.json, and profiles/parent_insert_profile.json
from the parent build).
"""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def clock(parts, name, fn):
    t0 = time.perf_counter()
    out = fn()
    parts[name] = parts.get(name, 0.0) + (time.perf_counter() - t0) * 1e3
    return out


def spread(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--k", type=int, default=40)
    ap.add_argument("--stars", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-host-route", action="store_true")
    ap.add_argument("--host-functions", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import sph_code_amd.compat as nsc
    from sph_code_amd import ics
    from sph_code_amd.sim import Simulation

    host_fn = nsc
    if a.host_functions:
        spec = importlib.util.spec_from_file_location("sph_code_amd._compat_host", a.host_functions)
        host_fn = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(host_fn)
    s = dict(ics.two_phase(a.n, size_scale=ics.bench_size_scale(a.n)))
    rs = np.random.RandomState(3)
    pt = np.array(s["particle_type"], dtype=np.float64)
    mass = np.array(s["mass"], dtype=np.float64)
    stars = np.sort(rs.choice(np.nonzero(pt == 0)[0], a.stars, replace=False)).astype(np.int64)
    pt[stars] = 1.0
    mass[stars] = 20.0 * nsc.solar_mass
    s.update(particle_type=pt, mass=mass)
    has = hasattr(Simulation, "supernova_explosion")
    res = dict(tool="insert_rate", n=a.n, k=a.k, stars=a.stars, repeats=a.repeats, build=nsc.context().build_info()["library"],
               has_resident_call=has)
    d_0, t_cmb = None, nsc.t_cmb

    def settle(sim):
        sim.ctx.check(sim.ctx.lib.sphx_sync(sim.ctx.h))                  # (the step is queued, not waited for)

    if not a.skip_host_route:
        runs, totals = [], []
        for it in range(a.repeats + 1):                                   # (the first pass warms the buffers up and is dropped)
            sim = Simulation(s, n_neigh=a.k, with_species=True)
            sim.step(1)
            settle(sim)
            p = {}
            t0 = time.perf_counter()
            st = clock(p, "download", sim.download)
            comp = clock(p, "download_composition", sim.download_composition)
            d_0 = float(np.median(st["sizes"][stars]))
            np.random.seed(11)
            ex = clock(p, "supernova_explosion", lambda: host_fn.supernova_explosion(comp["mass"], st["points"], st["velocities"],
                                                                                     st["E_internal"], stars, comp["f_un"], d_0=d_0))
            state = dict(st, particle_type=pt, **comp)
            new = clock(p, "supernova_insert", lambda: host_fn.supernova_insert(state, ex, t_cmb))
            up = {k_: new[k_] for k_ in ("points", "velocities", "E_internal", "T", "mass", "f_un", "mu_array", "gamma_array", "particle_type")}
            cur = clock(p, "new_simulation", lambda: Simulation(up, n_neigh=a.k, with_species=True))
            clock(p, "step_before_a_phase", lambda: (cur.step(1), settle(cur)))
            p["total"] = (time.perf_counter() - t0) * 1e3
            if it:
                runs.append(p); totals.append(p["total"])
        res["host_route"] = dict(ms_host={k_: float(np.median([r[k_] for r in runs])) for k_ in runs[0]}, ms_host_total=spread(totals),
                                 totals=totals, rows_appended=int(len(new["mass"]) - a.n))

    if has:
        host, dev, outs = [], [], []
        for it in range(a.repeats + 1):
            sim = Simulation(s, n_neigh=a.k, with_species=True)
            sim.step(1)
            settle(sim)
            if d_0 is None:
                d_0 = float(np.median(sim.download()["sizes"][stars]))
            np.random.seed(11)
            t0 = time.perf_counter()
            ev = sim.supernova_explosion(stars, d_0, t_cmb)
            ms = (time.perf_counter() - t0) * 1e3
            if it:
                host.append(ms); dev.append(sim.insert_timing())
                outs.append(dict(n_dust=ev["n_dust"], n_gas=ev["n_gas"], info=ev["info"]))
        med = {k_: float(np.median([t[k_] for t in dev])) for k_ in dev[0]}
        res["resident"] = dict(insert_device_ms=med, insert_device_ms_total=spread([sum(t.values()) for t in dev]), ms_host_call=spread(host),
                               host_calls=host, runs=outs, same_every_repeat=all(o == outs[0] for o in outs))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
