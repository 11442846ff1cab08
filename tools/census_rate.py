#!/usr/bin/env python3
"""Cost of what the driver reports every pass and saves at the end (code_running.py:341, 465-468, 616-622, 636, 656-664) on
the 1e6 polytrope and on the two-phase cube: Simulation.census, dust_temperatures, supernova_schedule and run_outputs on
the resident state, against the host route a user had to take before they existed.

Per workload: N particles with a seeded 15-species composition and seeded stellar ages, two steps.

  host route   download(), download_composition(), then the driver's statements in NumPy: the masses and counts by type,
               star_massfrac, star_numfrac, dust_temps, the total mass, the three by-species sums, the AGB rows, and the
               quantities of Simulation.diagnostics().  Only entry points older than Simulation.census: the tool runs
               unchanged on a build without it (an older checkout), where it is the baseline.  Host clock per part.
  resident     (where the library has it) per repeat: the host clock of census(), dust_temperatures(),
               supernova_schedule() and run_outputs(), the device time per stage of the census (prepare | chunk_sums |
               totals | read_back), and the totals of every repeat, which must agree bit for bit.

Prints one JSON line; --out FILE (meant for profiles/latest_census_profile.json, and profiles/parent_census_profile.json from
the parent build)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S = 15


def clock(parts, name, fn):
    t0 = time.perf_counter()
    out = fn()
    parts[name] = parts.get(name, 0.0) + (time.perf_counter() - t0) * 1e3
    return out


def spread(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def numpy_block(nsc, st, comp, pt, ages, parts):
    """The driver's statements on host arrays, timed part by part."""
    mass, f_un, T = comp["mass"], comp["f_un"], st["T"]
    mu_specie, solar_mass = nsc.mu_specie, nsc.solar_mass

    def fracs():
        star_massfrac = float(np.sum(mass[pt == 1])) / np.sum(mass[pt != 2])
        star_numfrac = float(len(pt[pt == 1])) / float(len(pt[pt != 2]))
        return star_massfrac, star_numfrac, T[pt == 2], np.sum(mass)
    out = clock(parts, "numpy_fractions_dust_temps_total", fracs)

    def species():
        return [np.sum((((f_un * mu_specie)[pt == t].T / np.sum((f_un * mu_specie)[pt == t], axis=1)) * mass[pt == t]).T, axis=0)
                for t in (0, 1, 2)]
    clock(parts, "numpy_by_species", species)

    def agb():
        cond = ((pt == 1) & (mass / solar_mass > 1.) & (mass / solar_mass < 7.))
        fm = (f_un * mu_specie)[cond]
        return mass[cond], nsc.luminosity_relation(mass[cond] / solar_mass, lifetime=1) * 1e10 * nsc.year - ages[cond], \
            np.sum(fm.T[6:], axis=0) / np.sum(fm, axis=1), (fm.T / np.sum(fm, axis=1)).T
    clock(parts, "numpy_agb", agb)

    def diag():
        mt = mass.sum()
        return (st["total_accel"] * mass[:, None]).sum(axis=0) / mt, (st["velocities"] * mass[:, None]).sum(axis=0), \
            0.5 * float((mass * (st["velocities"] ** 2).sum(axis=1)).sum()), float(st["E_internal"].sum())
    clock(parts, "numpy_diagnostics", diag)
    return out


def run(name, s, a, nsc, Simulation):
    pt = np.array(s["particle_type"], dtype=np.float64)
    n = pt.shape[0]
    rs = np.random.RandomState(12)
    # the workloads carry no stars: every 50th row becomes one of 0.5 .. 20 solar masses, with an age
    s = dict(s)
    pt[::50] = 1.0
    mass = np.array(s["mass"], dtype=np.float64)
    mass[::50] = np.exp(rs.uniform(np.log(0.5), np.log(20.0), size=mass[::50].shape[0])) * nsc.solar_mass
    s["particle_type"], s["mass"] = pt, mass
    f_un = rs.rand(n, S) + 1e-3
    s["f_un"] = f_un
    ages = np.where(pt == 1, rs.uniform(0., 1e9, size=n) * nsc.year, -1.0)
    has = hasattr(Simulation, "census")
    res = dict(n=int(n), has_resident_call=has, n_star=int(np.count_nonzero(pt == 1)), n_dust=int(np.count_nonzero(pt == 2)))

    def stepped():
        sim = Simulation(s, n_neigh=a.k, with_species=True)
        if has:
            sim.set_star_ages(ages)
        sim.step(2)
        sim.ctx.check(sim.ctx.lib.sphx_sync(sim.ctx.h))
        return sim

    sim = stepped()
    if not a.skip_host_route:
        runs, totals = [], []
        for it in range(a.repeats + 1):                                   # (the first pass warms the buffers up and is dropped)
            p = {}
            t0 = time.perf_counter()
            st = clock(p, "download", sim.download)
            comp = clock(p, "download_composition", sim.download_composition)
            numpy_block(nsc, st, comp, pt, ages, p)
            p["total"] = (time.perf_counter() - t0) * 1e3
            if it:
                runs.append(p); totals.append(p["total"])
        nbytes = sum(v.nbytes for v in list(st.values()) + list(comp.values()) if isinstance(v, np.ndarray))
        res["host_route"] = dict(ms_host={k_: float(np.median([r[k_] for r in runs])) for k_ in runs[0]}, ms_host_total=spread(totals),
                                 bytes_downloaded=int(nbytes))
    if has:
        host, dev, outs = [], [], []
        for it in range(a.repeats + 1):
            p = {}
            cen = clock(p, "census", sim.census)
            tm = sim.census_timing()
            clock(p, "dust_temperatures", sim.dust_temperatures)
            clock(p, "supernova_schedule", sim.supernova_schedule)
            clock(p, "run_outputs", lambda: sim.run_outputs(0.0))
            if it:
                host.append(p); dev.append(tm)
                outs.append([cen["total_mass"], cen["star_massfrac"], cen["kinetic"]] + cen["gas_mass_by_species"].tolist())
        res["resident"] = dict(device_ms={k_: float(np.median([t[k_] for t in dev])) for k_ in dev[0]},
                               device_ms_total=spread([sum(t.values()) for t in dev]),
                               ms_host_call={k_: float(np.median([h[k_] for h in host])) for k_ in host[0]},
                               same_every_repeat=all(o == outs[0] for o in outs))
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--k", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-host-route", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import sph_code_amd.compat as nsc
    from sph_code_amd import ics
    from sph_code_amd.sim import Simulation

    scale = ics.bench_size_scale(a.n)
    res = dict(tool="census_rate", n=a.n, k=a.k, repeats=a.repeats, species=S, build=nsc.context().build_info()["library"])
    res["polytrope"] = run("polytrope", dict(ics.polytrope_sphere(a.n, size_scale=scale)), a, nsc, Simulation)
    res["two_phase"] = run("two_phase", dict(ics.two_phase(a.n, size_scale=scale)), a, nsc, Simulation)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
