#!/usr/bin/env python3
"""Rate of supernova_destruction (include/sphx.h sphx_supernova_destruction) on the two-phase cube.

The N-particle two-phase cube (a tenth of the particles dust) after one step, its exact neighbour list from
compat.neighbors at the positions the step ended at, and seeded dust the way tests/golden/make_golden_dust.py draws it:
dust masses x U(0.5, 2) with crit_mass their median, dust f_un uniform over columns 7..14, velocities + N(0, 5e4 m/s),
sizes = the kNN radius (the dust's x U(0.6, 1.2)), densities = critical_density 10^U(-1, 2.5) under guard="fraction" (the
cap and the guard both act) or critical_density 10^U(-53.5, -49.5) under guard="count".  One warm-up call, then --repeats
calls, each timed by the library's HIP events on its stream (sphx_dust_last_timing: inputs going up, records and list |
reverse list | dust pass | row pass and outputs coming back) and by the host clock around the whole synchronous call.
Medians are reported.

  pairs                  (gas row, dust entry) pairs = the reverse list's entries
  dust_pairs_per_s       pairs over the dust pass's time        row_pairs_per_s   pairs over the row stage's time
  list_entries_per_s     N K list entries over the first stage's time
  particle_calls_per_s   N over the device time of the whole call, and over the host clock

Prints one JSON line; --out FILE (meant for profiles/latest_dust_profile.json).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--k", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--guard", default="fraction", choices=("count", "fraction"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import sph_code_amd.compat as nsc
    from sph_code_amd import ics
    from sph_code_amd.sim import Simulation

    s = ics.two_phase(a.n, size_scale=ics.bench_size_scale(a.n))
    sim = Simulation(s, n_neigh=a.k)
    sim.step(1)
    st = sim.download()
    pts = np.ascontiguousarray(st["points"])
    nb, _, _, _, h = nsc.neighbors(pts, np.inf, a.k)
    rs = np.random.RandomState(1)
    pt = np.asarray(s["particle_type"], dtype=np.float64)
    mass = np.array(s["mass"], dtype=np.float64)
    dust = pt == 2
    nd = int(dust.sum())
    mass[dust] *= rs.uniform(0.5, 2.0, nd)
    crit_mass = float(np.median(mass[dust]))
    f_un = np.array(s["f_un"], dtype=np.float64)
    fd = np.zeros((nd, f_un.shape[1]))
    fd[:, 7:15] = rs.uniform(0.0, 1.0, (nd, 8))
    f_un[dust] = fd / np.sum(fd, axis=1)[:, None]
    mu = np.sum(f_un * nsc.mu_specie, axis=1) / np.sum(f_un, axis=1)
    vel = np.asarray(st["velocities"], dtype=np.float64) + rs.normal(0.0, 5e4, (a.n, 3))
    sizes = np.array(h, dtype=np.float64)
    sizes[dust] *= rs.uniform(0.6, 1.2, nd)
    lo, hi = (-1.0, 2.5) if a.guard == "fraction" else (-53.5, -49.5)
    dens = nsc.critical_density * 10.0 ** rs.uniform(lo, hi, a.n)
    args = (pts, vel, nb, mass, f_un, mu, sizes, dens, pt)
    kw = dict(crit_mass=crit_mass, guard=a.guard, full=True)
    out = nsc.supernova_destruction(*args, **kw)                          # warm-up: buffers
    host, dev = [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        out = nsc.supernova_destruction(*args, **kw)
        host.append((time.perf_counter() - t0) * 1e3)
        dev.append(nsc.dust_last_timing())
    med = {k_: float(np.median([t[k_] for t in dev])) for k_ in dev[0]}
    valid = (nb >= 0) & (nb < a.n)
    pairs = int(np.count_nonzero(valid & (pt == 0)[:, None] & dust[np.where(valid, nb, 0)]))
    ms_dev = sum(med.values())
    res = dict(tool="dust_rate", n=a.n, k=a.k, species=int(f_un.shape[1]), dust_particles=nd, repeats=a.repeats, guard=a.guard,
               crit_mass=crit_mass, build=nsc.context().build_info()["library"],
               ms_upload=med["upload"], ms_reverse=med["reverse"], ms_dust=med["dust"], ms_rows=med["rows"],
               ms_device=ms_dev, ms_host_call=float(np.median(host)), pairs=pairs,
               list_entries_per_s=float(a.n) * a.k / (med["upload"] * 1e-3),
               dust_pairs_per_s=pairs / (med["dust"] * 1e-3), row_pairs_per_s=pairs / (med["rows"] * 1e-3),
               particle_calls_per_s_device=a.n / (ms_dev * 1e-3), particle_calls_per_s_host=a.n / (np.median(host) * 1e-3),
               counts=out[2], destruction_nonzero=int(np.count_nonzero(out[0])), reuptake_nonzero=int(np.count_nonzero(out[1])),
               destruction_max=float(out[0].max()))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
