#!/usr/bin/env python3
"""Cost of the gravitational potential and the energy budget (include/sphx.h: sphx_gravity_direct_pot,
sphx_gravity_tree_pot, sphx_state_gravity_potential) against the sums without it and against the host route a user had
to take before they existed.  Polytrope, seeded masses, eps = median(h) of the step.

  direct, 1e5 particles   host time of the array calls without phi (grav_force_*) and with it (grav_potential_*(return_accel=
  tree,   1e6 particles   True): the same uploads, grid and walk, n doubles more to download) and their ratio - the phi-on /
  (ws 1, order 2)         phi-off comparison of one call; the library times no stage of the calls without phi, so there is no
                          device-only figure for them | device time per stage of the array call with phi (upload | build |
                          sum = the kernel or walk alone | download) | device time per stage of
                          Simulation.gravity_potential() (upload = gather + median | build | sum = walk + totals | download) |
                          host time of Simulation.energy() | for orientation, the step's own gravity (stats ms_gravity with
                          the per-pass events on: median + pyramid of the step's grid + walk; another grid, not a ratio)
  host route, 1e5 only    download(), download_composition(), then U = 1/2 sum m phi by a chunked NumPy sum over all pairs
                          and the kinetic and internal energy.  Only entry points older than the potential: the tool runs
                          unchanged on a build without it (an older checkout), where it times the host route alone.

Prints one JSON line; --out FILE (meant for profiles/latest_gravpot_profile.json, and profiles/parent_gravpot_profile.json from
the parent build)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

G = 6.67430e-11


def spread(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def numpy_energy(st, comp, chunk=64):
    """U, kinetic, internal of a downloaded state: the chunked sum over all pairs, self left out by index."""
    p, m, eps = st["points"], comp["mass"], float(np.median(st["sizes"]))
    n = len(m)
    cols = np.arange(n)
    U = 0.0
    for a in range(0, n, chunk):
        d = p[None, :, :] - p[a:a + chunk, None, :]
        r2 = np.sum(d * d, axis=2) + eps * eps
        with np.errstate(all="ignore"):
            t = np.where((r2 > 0) & (cols[None, :] != cols[a:a + chunk, None]), m[None, :] / np.sqrt(r2), 0.0)
        U += -0.5 * G * float(np.sum(m[a:a + chunk] * np.sum(t, axis=1)))
    return U, 0.5 * float((m * (st["velocities"] ** 2).sum(axis=1)).sum()), float(st["E_internal"].sum())


def run(mode, n, a, nsc, ics, Simulation, host_route):
    s = dict(ics.polytrope_sphere(n, size_scale=ics.bench_size_scale(n)))
    s["mass"] = np.array(s["mass"], dtype=np.float64) * np.random.RandomState(1).uniform(0.5, 1.5, n)
    has = hasattr(Simulation, "gravity_potential")
    res = dict(n=int(n), mode=mode, has_potential=has)
    sim = Simulation(s, n_neigh=a.k, gravity=mode, G=G)
    sim.ctx.set_timing_detail(True)
    sim.step(1)
    sim.reset_stats()
    sim.step(a.repeats)
    stt = sim.stats()
    res["step_gravity_device_ms"] = float(stt["ms_gravity"]) / max(1, int(stt["detail_steps"]))
    st, comp = sim.download(), sim.download_composition()
    m, p, h = comp["mass"], np.ascontiguousarray(st["points"]), st["sizes"]
    force = nsc.grav_force_direct if mode == "direct" else nsc.grav_force_tree
    host_off = [timed(lambda: force(m, p, h, G=G))[1] for _ in range(a.repeats + 1)][1:]
    res["array_call_host_ms_without_phi"] = spread(host_off)
    if has:
        pot = nsc.grav_potential_direct if mode == "direct" else nsc.grav_potential_tree
        host_on, dev_on = [], []
        for it in range(a.repeats + 1):
            host_on.append(timed(lambda: pot(m, p, h, G=G, return_accel=True))[1])
            dev_on.append(nsc.gravpot_last_timing())
        res["array_call_host_ms_with_phi"] = spread(host_on[1:])
        res["array_call_device_ms_with_phi"] = {k_: float(np.median([t[k_] for t in dev_on[1:]])) for k_ in dev_on[0]}
        e_ms, dev, outs = [], [], []
        for it in range(a.repeats + 1):
            e, ms = timed(sim.energy)
            e_ms.append(ms); dev.append(sim.gravpot_timing()); outs.append((e["potential"], e["total"], e["virial"]))
        res["energy_host_ms"] = spread(e_ms[1:])
        res["potential_device_ms"] = {k_: float(np.median([t[k_] for t in dev[1:]])) for k_ in dev[0]}
        res["array_call_host_phi_on_over_off"] = res["array_call_host_ms_with_phi"]["median"] / res["array_call_host_ms_without_phi"]["median"]
        res["energy"] = dict(zip(("potential", "total", "virial"), outs[0]))
        res["same_every_repeat"] = all(o == outs[0] for o in outs)
    if host_route:
        t0 = time.perf_counter()                                          # (O(N^2) in NumPy: minutes at 1e5; one pass)
        (st2, t_dl), (comp2, t_dc) = timed(sim.download), timed(sim.download_composition)
        out, t_np = timed(lambda: numpy_energy(st2, comp2))
        res["host_route"] = dict(ms_host=dict(download=t_dl, download_composition=t_dc, numpy_sum=t_np,
                                              total=(time.perf_counter() - t0) * 1e3), U=out[0])
    print(mode, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-direct", type=int, default=100000)
    ap.add_argument("--n-tree", type=int, default=1000000)
    ap.add_argument("--k", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-host-route", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import sph_code_amd.compat as nsc
    from sph_code_amd import ics
    from sph_code_amd.sim import Simulation

    res = dict(tool="gravpot_rate", k=a.k, repeats=a.repeats, build=nsc.context().build_info()["library"])
    res["direct"] = run("direct", a.n_direct, a, nsc, ics, Simulation, not a.skip_host_route)
    res["tree"] = run("tree", a.n_tree, a, nsc, ics, Simulation, False)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
