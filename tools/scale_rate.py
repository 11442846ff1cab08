#!/usr/bin/env python3
"""Cost of the closing block of the time loop (code_running.py:493-540: the global length scale d and the adapted sizes) on
the 1e6 polytrope and on the two-phase cube: Simulation.length_scale on the resident state, against the host route a
user had to take before it existed.

Per workload: N particles, two steps (so that the call has a densities_0 from a first call behind the first step).

  host route   download(), neighbors(), then the driver's statements in NumPy: np.sum over the squared velocities and
               positions, np.percentile over the slow rows, d; np.bincount over the list for the reverse counts (the
               driver's own list comprehension over np.unique is quadratic and is not what anyone would run), the count
               of each row's entries, np.exp / np.nan_to_num and the three masked assignments.  The new sizes then have
               nowhere to go: no entry point uploads sizes into a running Simulation, so the route ends with the arrays on
               the host.  Only entry points older than Simulation.length_scale: the tool runs unchanged on a build
               without it (an older checkout), where it is the baseline.  Host clock per part.
  resident     (where the library has it) per repeat Simulation.length_scale(apply=True): the host clock of the call and
               the device time per stage (keys | select | reverse_counts | adapt | write_back); d, the slow rows and the
               counts of every repeat, which must agree.

Prints one JSON line; --out FILE (meant for profiles/latest_scale_profile.json, and profiles/parent_scale_profile.json from
the parent build).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_INT_PER_PARTICLE = 40
RAISE_FACTOR = 715               # drv:59


def clock(parts, name, fn):
    t0 = time.perf_counter()
    out = fn()
    parts[name] = parts.get(name, 0.0) + (time.perf_counter() - t0) * 1e3
    return out


def spread(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def numpy_block(st, nb, densities_0, pt, parts):
    """drv:493-538 on host arrays, timed part by part -> (d, sizes)."""
    n = pt.shape[0]

    def scale():
        vel_condition = np.sum(st["velocities"] ** 2, axis=1)
        dist_sq = np.sum(st["points"] ** 2, axis=1)
        slow = vel_condition < 80000 ** 2
        max_dist = np.percentile(dist_sq[slow], 90)
        return (max_dist ** (3. / 2.) / np.count_nonzero(slow) / 0.9 * N_INT_PER_PARTICLE) ** (1. / 3.)
    d = clock(parts, "numpy_percentile_and_d", scale)

    def counts():
        ok = nb < n
        return np.bincount(nb[ok], minlength=n), np.count_nonzero(ok, axis=1)
    cnt, nontriv = clock(parts, "numpy_bincount", counts)

    def adapt():
        sizes = np.array(st["sizes"])
        rho = st["densities"]
        with np.errstate(all="ignore"):
            new_smoothing = (np.exp(np.nan_to_num(-(rho - densities_0) / (3 * rho))) * 2) / 2. + (cnt + nontriv - 1 < 2) * 0.1
            sizes[pt == 0] = (new_smoothing * sizes)[pt == 0]
            sizes[(pt == 0) & (sizes > d)] = d
            sizes[pt == 2] = d / RAISE_FACTOR ** (1. / 3.)
        return sizes
    return d, clock(parts, "numpy_elementwise", adapt)


def run(name, s, a, Simulation):
    pt = np.array(s["particle_type"], dtype=np.float64)
    has = hasattr(Simulation, "length_scale")
    res = dict(n=int(pt.shape[0]), has_resident_call=has)

    def stepped():
        """A Simulation behind its second step, and the first step's densities."""
        sim = Simulation(s, n_neigh=a.k)
        sim.step(1)
        rho1 = sim.download()["densities"]
        if has:
            sim.length_scale(N_INT_PER_PARTICLE, RAISE_FACTOR)
        sim.step(1)
        sim.ctx.check(sim.ctx.lib.sphx_sync(sim.ctx.h))                 # (the step is queued, not waited for)
        return sim, rho1

    if not a.skip_host_route:
        runs, totals = [], []
        for it in range(a.repeats + 1):                                   # (the first pass warms the buffers up and is dropped)
            sim, rho1 = stepped()
            p = {}
            t0 = time.perf_counter()
            st = clock(p, "download", sim.download)
            nb = clock(p, "neighbors_download", sim.neighbors)
            d, sizes = numpy_block(st, nb, rho1, pt, p)
            p["total"] = (time.perf_counter() - t0) * 1e3
            if it:
                runs.append(p); totals.append(p["total"])
        res["host_route"] = dict(ms_host={k_: float(np.median([r[k_] for r in runs])) for k_ in runs[0]}, ms_host_total=spread(totals),
                                 d=float(d), bytes_downloaded=int(sum(v.nbytes for v in st.values() if isinstance(v, np.ndarray)) + nb.nbytes))
    if has:
        host, dev, outs = [], [], []
        for it in range(a.repeats + 1):
            sim, _ = stepped()
            t0 = time.perf_counter()
            r = sim.length_scale(N_INT_PER_PARTICLE, RAISE_FACTOR)
            ms = (time.perf_counter() - t0) * 1e3
            if it:
                host.append(ms); dev.append(sim.scale_timing())
                outs.append(dict(d=r["d"], n_slow=r["n_slow"], counts=r["counts"]))
        res["resident"] = dict(device_ms={k_: float(np.median([t[k_] for t in dev])) for k_ in dev[0]},
                               device_ms_total=spread([sum(t.values()) for t in dev]), ms_host_call=spread(host), runs=outs[:1],
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
    res = dict(tool="scale_rate", n=a.n, k=a.k, repeats=a.repeats, n_int_per_particle=N_INT_PER_PARTICLE, raise_factor=RAISE_FACTOR,
               build=nsc.context().build_info()["library"])
    res["polytrope"] = run("polytrope", dict(ics.polytrope_sphere(a.n, size_scale=scale)), a, Simulation)
    res["two_phase"] = run("two_phase", dict(ics.two_phase(a.n, size_scale=scale)), a, Simulation)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
