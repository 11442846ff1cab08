#!/usr/bin/env python3
"""Cost of the radiative block of the time loop (code_running.py:247-316) on the two-phase cube.

The N-particle two-phase cube after one step; 32 seeded gas particles retyped as stars of 10^U(-0.3, 1.6) solar masses;
the targets selected by the reference's rule (compat.rad_setup: about N^0.35 of them); a seeded ionised composition for
the gas the way tools/cool_rate.py draws it; E_internal = N_PART gamma k T; d such that the median h(m) is the median kNN
radius.

  host route   download the state, compat.rad_transfer, the chemistry of nsc:976-1012 and the bookkeeping of drv:258-311 in
               float64 NumPy, compat.neighbors, compat.rad_cooling, a new Simulation from the result.  Only entry points
               older than the radiative array calls: the tool runs unchanged on a build without them, where it is the
               baseline.  Host clock per part, and the two array calls' own stage timers.
  resident     (where the library has it) Simulation.rad_phase again and again on the state it leaves: its stage timer
               (gather | transfer | ionise + heat | cooling | bookkeeping and write-back) and the host clock, beside the sum
               of the kernel stages of the two physics array calls on the same cloud (the expectation's first term).
  array route  (where the library has it) compat.rad_phase's stages one by one on the same arrays: host clock per part
               and sphx_radphase_last_timing's stages for the three elementwise calls, with the bandwidth the row kernels
               reach (bytes they must read and write over the kernel stage's time).

Medians of --repeats after one warm-up.  Prints one JSON line; --out FILE (meant for profiles/latest_radphase_profile.json).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from cool_rate import composition  # noqa: E402

T_MAX = 1e4
T_CMB = 2.732
SB = 5.6703744191844314e-08
CROSS_GAS = np.array([6.3e-22, 6.3e-22, 6.3e-22, 1e-60, 1e-60, 1.e-60, 6.65e-60 * 80] + [0.] * 8) / 80. + 1e-80


def clock(parts, name, fn):
    t0 = time.perf_counter()
    out = fn()
    parts.setdefault(name, []).append((time.perf_counter() - t0) * 1e3)
    return out


def medians(parts):
    return {k_: float(np.median(v)) for k_, v in parts.items()}


def tables_of(nsc, f, cs):
    tot = np.sum(f, axis=1)
    return np.sum(f * nsc.mu_specie, axis=1) / tot, np.sum(f * nsc.gamma, axis=1) / tot, np.sum(f * cs, axis=1) / tot


def clamps(nsc, E, T, mass, mu, gam):
    lo = T_CMB * (gam * mass * nsc.k) / (mu * nsc.m_h)
    hi = T_MAX * (gam * mass * nsc.k) / (mu * nsc.m_h)
    E = np.where(E < lo, lo, E)
    E = np.where(E > hi, hi, E)
    return E, np.where(T >= T_MAX, T_MAX, np.where(T < T_CMB, T_CMB, T))


def coefficient(x):
    x = np.nan_to_num(x)
    return np.where(x >= 0, x + 1., np.exp(np.minimum(x, 0.)))


def numpy_ionise(nsc, f, pt, mass, lf2, frac_dest, ppj):
    """nsc:976-1012 in float64 NumPy."""
    ns = pt != 1
    g = f[ns]
    mols = mass[ns] / np.sum(g * nsc.mu_specie * nsc.amu, axis=1)
    wi = (g * CROSS_GAS)[:, :3] / np.sum(g * CROSS_GAS, axis=1)[:, None]
    total = g[:, :3] * mols[:, None]
    fr = np.nan_to_num(0.99 - 0.99 * np.exp(-np.nan_to_num(wi * frac_dest[:3] * (ppj * lf2)[:, None] / total)))
    fr[total / nsc.amu < 1e-10] = 0.
    fr[total / nsc.amu < 0] = 0.99
    p = g[:, :3] * fr
    new = g.copy()
    new[:, 0] -= p[:, 0]; new[:, 1] -= p[:, 1]; new[:, 2] += 2. * p[:, 0] - p[:, 2]
    new[:, 3] += p[:, 2]; new[:, 4] += p[:, 1]; new[:, 5] += p[:, 2] + p[:, 1]
    out = f.copy()
    out[ns] = new
    return out / np.sum(out, axis=1)[:, None]


def numpy_heat(nsc, f, pt, mass, mu0, E, T, lf2, cs):
    """drv:258-273 in float64 NumPy."""
    mu, gam, cross = tables_of(nsc, f, cs)
    gas = pt == 0
    E, T = E.copy(), T.copy()
    E[gas] *= coefficient(lf2[pt[pt != 1] == 0] / E[gas])
    T[gas] = E[gas] / ((mass / (nsc.m_h * mu0)) * gam * nsc.k)[gas]
    return (mu, gam, cross) + clamps(nsc, E, T, mass, mu, gam)


def numpy_cool(nsc, f, energy, pt, mass, sizes, E, T, vel, lf2, mom, cs, dt, cooling_timescale):
    """drv:283-311 in float64 NumPy."""
    mu, gam, cross = tables_of(nsc, f, cs)
    gas, dust = pt == 0, pt == 2
    n_part = mass / (nsc.m_h * mu)
    E, T, vel = E.copy(), T.copy(), vel.copy()
    c1 = coefficient(-(energy * n_part)[gas] / E[gas]) * np.exp(-dt / cooling_timescale * np.sqrt(T[gas] / 1e4))
    E[gas] *= c1
    T[gas] = E[gas] / (n_part * gam * nsc.k)[gas]
    optd = 1. - np.exp(-(n_part * cross) * 9. / (4 * np.pi * sizes ** 2))
    T[dust] = (lf2[pt[pt != 1] == 2] / (optd * 4 * np.pi * sizes ** 2 * SB * 1e-5 * dt)[dust] + T_CMB ** (1. / 6.)) ** (1. / 6.)
    E[dust] = (n_part * nsc.k * T * gam)[dust]
    vel[pt != 1] += mom
    return (mu, gam, cross) + clamps(nsc, E, T, mass, mu, gam) + (vel,)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--k", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--stars", type=int, default=32)
    ap.add_argument("--skip-host-route", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import sph_code_amd.compat as nsc
    from sph_code_amd import ics
    from sph_code_amd.sim import Simulation

    s = dict(ics.two_phase(a.n, size_scale=ics.bench_size_scale(a.n)))
    rs = np.random.RandomState(1)
    pt = np.array(s["particle_type"], dtype=np.float64)
    mass = np.array(s["mass"], dtype=np.float64)
    stars = rs.choice(np.nonzero(pt == 0)[0], a.stars, replace=False)
    pt[stars] = 1.0
    mass[stars] = nsc.solar_mass * 10.0 ** rs.uniform(-0.3, 1.6, a.stars)
    gas = pt == 0
    f_un = np.array(s["f_un"], dtype=np.float64)
    f_un[gas] = composition(rs, int(gas.sum()), f_un.shape[1])
    T = np.array(s["T"], dtype=np.float64)
    T[gas] = 10.0 ** rs.uniform(1.0, 4.5, int(gas.sum()))
    mu = np.sum(f_un * nsc.mu_specie, axis=1) / np.sum(f_un, axis=1)
    gam = np.sum(f_un * nsc.gamma, axis=1) / np.sum(f_un, axis=1)
    s.update(particle_type=pt, mass=mass, f_un=f_un, T=T, mu_array=mu, gamma_array=gam, E_internal=gam * mass * nsc.k * T / (mu * nsc.m_h))
    sim = Simulation(s, n_neigh=a.k, **({"with_species": True} if hasattr(Simulation, "rad_phase") else {}))      # (the resident phase needs the rows)
    sim.step(1)
    dt = float(nsc.dt_0) * 1e-3
    cooling_timescale = 4.0 * dt
    lo, hi = 50e-10, 5000e-10
    cs = CROSS_GAS + nsc.mu_specie * nsc.amu / nsc.mineral_densities * (3. / 4.) * -(hi ** -0.5 - lo ** -0.5) / (hi ** 0.5 - lo ** 0.5)
    # the setup of nsc:897-921 with every star a source (parent builds have no compat.rad_setup)
    star_m = mass[pt == 1] / nsc.solar_mass
    src, lum = np.nonzero(pt == 1)[0], np.where(star_m < 0.7, 0.35 * star_m ** 2.62, 1.02 * star_m ** 3.92)
    others = np.nonzero(pt != 1)[0]
    dst = others[np.random.RandomState(7).rand(len(others)) < len(others) ** -0.65]
    frac_dest, ppj = np.array([0.96, 0.46, 0.74] + [0.0] * (f_un.shape[1] - 3)), 2.3e17
    if hasattr(nsc, "stellar_spectrum"):
        frac_dest, ppj = nsc.stellar_spectrum(mass[pt == 1])
    d = None
    host, array, dev, figures = {}, {}, {}, {}
    for rep in range(a.repeats + 1):
        parts_h, parts_a = ({}, {}) if rep == 0 else (host, array)          # (rep 0: warm-up, not kept)
        st = clock(parts_h, "download", sim.download)
        pts, vel = np.ascontiguousarray(st["points"]), np.ascontiguousarray(st["velocities"])
        sizes = np.asarray(st["sizes"], dtype=np.float64)
        E, T = np.asarray(st["E_internal"], dtype=np.float64), np.asarray(st["T"], dtype=np.float64)      # (as the step left them)
        cross0 = np.sum(f_un * cs, axis=1) / np.sum(f_un, axis=1)
        if not a.skip_host_route:
            lf2, mom, _ = clock(parts_h, "rad_transfer", lambda: nsc.rad_transfer(pts, pt, mass, sizes, cross0, mu, pts[src], lum, pts[dst], dt))
            dev.setdefault("host_rad", []).append(nsc.rad_last_timing())
            with np.errstate(all="ignore"):
                f1 = clock(parts_h, "numpy_ionise", lambda: numpy_ionise(nsc, f_un, pt, mass, lf2, frac_dest, ppj))
                mu1, g1, cr1, E1, T1 = clock(parts_h, "numpy_heat", lambda: numpy_heat(nsc, f1, pt, mass, mu, E, T, lf2, cs))
            nb, _, _, _, h = clock(parts_h, "neighbors", lambda: nsc.neighbors(pts, np.inf, a.k))
            if d is None:
                d = float(np.median(h) / np.median((mass / nsc.m_0) ** (1.0 / 3.0)))
            final, energy, _ = clock(parts_h, "rad_cooling", lambda: nsc.rad_cooling(pts, pt, mass, sizes, cr1, f1, nb, mu1, T1, dt, d=d))
            dev.setdefault("host_cool", []).append(nsc.cool_last_timing())
            with np.errstate(all="ignore"):
                res = clock(parts_h, "numpy_cool", lambda: numpy_cool(nsc, final, energy, pt, mass, sizes, E1, T1, vel, lf2, mom, cs, dt,
                                                                      cooling_timescale))
            new = dict(points=pts, velocities=res[5], total_accel=st["total_accel"], E_internal=res[3], T=res[4], mass=mass, f_un=final,
                       mu_array=res[0], gamma_array=res[1], particle_type=pt)
            clock(parts_h, "new_simulation", lambda: Simulation(new, n_neigh=a.k))
            figures["host_E_after"] = float(np.sum(res[3]))
        if hasattr(nsc, "rad_cool_bookkeeping"):
            if d is None:
                h = nsc.neighbors(pts, np.inf, a.k)[4]
                d = float(np.median(h) / np.median((mass / nsc.m_0) ** (1.0 / 3.0)))
            if a.skip_host_route:        # (otherwise the host route's list: both routes then do the same work)
                nb = sim.neighbors()
            cr0 = clock(parts_a, "cross_array", lambda: nsc.cross_array_of(f_un))
            lf2, mom, _ = clock(parts_a, "rad_transfer", lambda: nsc.rad_transfer(pts, pt, mass, sizes, cr0, mu, pts[src], lum, pts[dst], dt))
            f1 = clock(parts_a, "rad_ionise", lambda: nsc.rad_ionise(f_un, pt, mass, lf2, frac_dest, ppj))
            dev.setdefault("ionise", []).append(nsc.radphase_last_timing())
            mu1, g1, cr1, E1, T1, _ = clock(parts_a, "rad_heat_bookkeeping", lambda: nsc.rad_heat_bookkeeping(f1, pt, mass, mu, E, T, lf2, T_MAX))
            dev.setdefault("heat", []).append(nsc.radphase_last_timing())
            final, energy, _ = clock(parts_a, "rad_cooling", lambda: nsc.rad_cooling(pts, pt, mass, sizes, cr1, f1, nb, mu1, T1, dt, d=d))
            out = clock(parts_a, "rad_cool_bookkeeping", lambda: nsc.rad_cool_bookkeeping(final, energy, pt, mass, sizes, E1, T1, vel, lf2, mom, dt,
                                                                                         T_MAX, cooling_timescale))
            dev.setdefault("cool", []).append(nsc.radphase_last_timing())
            figures["array_E_after"] = out[6]["E_after"]
            figures["array_counts"] = {k_: v for k_, v in out[6].items() if k_ not in ("E_before", "E_after")}
    # ---- the resident call: one Simulation, the phase again and again on the state it leaves ----
    resident = {}
    if hasattr(sim, "rad_phase"):
        if d is None:
            h = nsc.neighbors(np.ascontiguousarray(sim.download()["points"]), np.inf, a.k)[4]
            d = float(np.median(h) / np.median((mass / nsc.m_0) ** (1.0 / 3.0)))
        wall, stages = [], []
        for rep in range(a.repeats + 1):
            t0 = time.perf_counter()
            tot = sim.rad_phase(dt, d, src, lum, dst, frac_dest, ppj, T_MAX, cooling_timescale)
            wall.append((time.perf_counter() - t0) * 1e3)
            stages.append(sim.radphase_timing())
        med = {k_: float(np.median([s_[k_] for s_ in stages[1:]])) for k_ in stages[0]}
        resident = dict(resident_stage_ms=med, resident_device_ms=sum(med.values()), resident_host_call_ms=float(np.median(wall[1:])),
                        resident_last_totals={k_: v for k_, v in tot.items()})
        if "host_rad" in dev and "host_cool" in dev:
            hr = {k_: float(np.median([t_[k_] for t_ in dev["host_rad"][1:]])) for k_ in dev["host_rad"][0]}
            hc = {k_: float(np.median([t_[k_] for t_ in dev["host_cool"][1:]])) for k_ in dev["host_cool"][0]}
            resident["expectation_kernel_stages_ms"] = hr["columns"] + hr["deposit"] + hc["rows"] + hc["gather"]
    n, S, g = a.n, f_un.shape[1], int(np.count_nonzero(pt != 1))
    stage = {name: {k_: float(np.median([t[k_] for t in v[1:]])) for k_ in v[0]} for name, v in dev.items()}
    # what each row kernel must move: the rows in (and out), the per-particle arrays in and out, the totals' terms
    moved = dict(ionise=8 * (2 * n * S + 2 * n + g + n / 2), heat=8 * (n * S + 5 * n + g + 5 * n + 6 * n),
                 cool=8 * (n * S + 9 * n + 4 * g + 8 * n + 6 * n))
    res = dict(tool="radphase_rate", n=n, k=a.k, species=S, stars=a.stars, targets=int(len(dst)), repeats=a.repeats, dt=dt,
               build=nsc.context().build_info()["library"], host_route_ms=medians(host), host_route_total_ms=sum(medians(host).values()),
               array_route_ms=medians(array), array_route_total_ms=sum(medians(array).values()), device_stage_ms=stage,
               kernel_tb_per_s={k_: moved[k_] / (stage[k_]["kernel"] * 1e-3) / 1e12 for k_ in moved if k_ in stage}, **figures, **resident)
    if "host_E_after" in res and "array_E_after" in res:
        res["E_after_relative_difference"] = abs(res["array_E_after"] - res["host_E_after"]) / abs(res["host_E_after"])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
