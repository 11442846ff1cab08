#!/usr/bin/env python3
"""Cost of the supernova event of the time loop (code_running.py:350-358) on the two-phase cube: the kicks and the event's
time step by Simulation.supernova_impulse on the resident state, against the host route a user had to take before it
existed.

The N-particle two-phase cube, one step; --stars gas rows drawn (seeded) and turned into 20 M_sun stars; mass_displaced
such that about --select gas rows of median mass reach the boundary (the reference's regime: a few hundred to a few
thousand rows).

  host route   download and download_composition, per star the reference's statement in NumPy (the squared distances, a
               full np.argsort over N, the mask, the cumulative sum, the kick), compat.crossing_time on neighbors(), then -
               the kicked velocities have to get back - a new Simulation from the result and the step it needs before a
               phase can run.  Only entry points older than Simulation.supernova_impulse: the tool runs unchanged on a
               build without it (an older checkout), where it is the baseline.  Host clock per part.
  resident     (where the library has it) per repeat Simulation.supernova_impulse on a state stepped once: the host clock
               of the call and the device time per stage of the selection (keys | bound | compact | sort | walk | kick, added
               up over the stars; the gather, the crossing time and the write-back are in the host clock only), the
               candidates and the selected rows per star.  Every repeat starts from a fresh Simulation of the same state, so
               the repeats do the same work.

The insertion of the new particles (drv:361-396) is not part of either route: the library does not have it yet.

Prints one JSON line; --out FILE (meant for profiles/latest_sn_profile.json, and profiles/parent_sn_profile.json from the
parent build).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SUPERNOVA_ENERGY = 1e44          # nsc:35
KICK_FRACTION = 0.736            # nsc:1200


def clock(parts, name, fn):
    t0 = time.perf_counter()
    out = fn()
    parts[name] = parts.get(name, 0.0) + (time.perf_counter() - t0) * 1e3
    return out


def spread(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def numpy_impulse(points, masses, ku, ptypes, mass_displaced, parts):
    """nsc:1192-1204 as written, timed statement by statement."""
    s = clock(parts, "numpy_distances", lambda: np.sum((points - points[ku]) ** 2, axis=1))
    order = clock(parts, "numpy_argsort", lambda: np.argsort(s))

    def rest():
        g = order[ptypes[order] == 0]
        sel = g[np.cumsum(masses[g]) < mass_displaced]
        vel = (2 * SUPERNOVA_ENERGY * KICK_FRACTION / np.sum(masses[sel])) ** 0.5
        d = points[sel] - points[ku]
        return (d.T / np.sum(d ** 2, axis=1) ** 0.5 * vel).T, sel
    return clock(parts, "numpy_select_and_kick", rest)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--k", type=int, default=40)
    ap.add_argument("--stars", type=int, default=1)
    ap.add_argument("--select", type=float, default=2000.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-host-route", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import sph_code_amd.compat as nsc
    from sph_code_amd import ics
    from sph_code_amd.sim import Simulation

    s = dict(ics.two_phase(a.n, size_scale=ics.bench_size_scale(a.n)))
    rs = np.random.RandomState(3)
    pt = np.array(s["particle_type"], dtype=np.float64)
    mass = np.array(s["mass"], dtype=np.float64)
    stars = np.sort(rs.choice(np.nonzero(pt == 0)[0], a.stars, replace=False)).astype(np.int64)
    pt[stars] = 1.0
    mass[stars] = 20.0 * nsc.solar_mass
    mass_displaced = float(a.select * np.median(mass[pt == 0]))
    s.update(particle_type=pt, mass=mass)
    res = dict(tool="sn_rate", n=a.n, k=a.k, stars=a.stars, gas_rows=int(np.sum(pt == 0)), repeats=a.repeats, mass_displaced=mass_displaced,
               build=nsc.context().build_info()["library"], has_resident_call=hasattr(Simulation, "supernova_impulse"))

    if not a.skip_host_route:
        runs, totals, selected = [], [], []
        for it in range(a.repeats + 1):                                   # (the first pass warms the buffers up and is dropped)
            sim = Simulation(s, n_neigh=a.k, with_species=True)
            sim.step(1)
            sim.ctx.check(sim.ctx.lib.sphx_sync(sim.ctx.h))             # (the step is queued, not waited for)
            p = {}
            t0 = time.perf_counter()
            st = clock(p, "download", sim.download)
            comp = clock(p, "download_composition", sim.download_composition)
            nb = clock(p, "neighbors_download", sim.neighbors)
            v = np.array(st["velocities"])
            sel_n = []
            for ku in stars:
                d_vels, sel = numpy_impulse(st["points"], comp["mass"], int(ku), pt, mass_displaced, p)
                v[sel] += d_vels
                sel_n.append(int(sel.shape[0]))
            ct = clock(p, "crossing_time", lambda: nsc.crossing_time(nb, v, st["sizes"], pt))
            dt_event = min(nsc.dt_0 / 100., ct)
            state = dict(points=st["points"], velocities=v, total_accel=st["total_accel"], E_internal=st["E_internal"], T=st["T"],
                         mass=comp["mass"], f_un=comp["f_un"], mu_array=comp["mu_array"], gamma_array=comp["gamma_array"], particle_type=pt)
            cur = clock(p, "new_simulation", lambda: Simulation(state, n_neigh=a.k, with_species=True))
            clock(p, "step_before_a_phase", lambda: (cur.step(1, fixed_dt=dt_event), cur.ctx.check(cur.ctx.lib.sphx_sync(cur.ctx.h))))
            p["total"] = (time.perf_counter() - t0) * 1e3
            if it:
                runs.append(p); totals.append(p["total"]); selected.append(sel_n)
        res["host_route"] = dict(ms_host={k_: float(np.median([r[k_] for r in runs])) for k_ in runs[0]}, ms_host_total=spread(totals),
                                 selected=selected[0], dt_event=float(dt_event))

    if res["has_resident_call"]:
        host, dev, outs = [], [], []
        for it in range(a.repeats + 1):
            sim = Simulation(s, n_neigh=a.k, with_species=True)
            sim.step(1)
            sim.ctx.check(sim.ctx.lib.sphx_sync(sim.ctx.h))
            t0 = time.perf_counter()
            ev = sim.supernova_impulse(stars, mass_displaced=mass_displaced)
            ms = (time.perf_counter() - t0) * 1e3
            if it:
                host.append(ms); dev.append(sim.sn_timing())
                outs.append(dict(selected=[int(x) for x in ev["sel_count"]], counts=ev["counts"], dt_event=ev["dt"], ct=ev["ct"]))
        med = {k_: float(np.median([t[k_] for t in dev])) for k_ in dev[0]}
        res["resident"] = dict(selection_device_ms=med, selection_device_ms_total=spread([sum(t.values()) for t in dev]),
                               ms_host_call=spread(host), runs=outs, same_every_repeat=all(o == outs[0] for o in outs))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
