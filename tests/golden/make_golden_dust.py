#!/usr/bin/env python3
"""Generate tests/golden/dust_<case>.npz: the reference's supernova_destruction (nsc:1211-1263) on seeded inputs.

CONTAINER-ONLY TOOL, a no-op (exit 0 with a message) where the reference is absent.  It loads the reference the way
make_golden_cool does (an in-memory Python-2 -> Python-3 transform; no reference text is stored) with ONE repair applied
in memory: the module's tuple of interpolants `intf` has 14 entries for the 15 species of
mu_specie, and the function raises a broadcast ValueError on its first contributing row; the reference's own
zero_function (intf[0]) is appended until len(intf) == len(mu_specie) - asserted.  None of the entries the reference
wrote changes.  The module globals crit_mass (the driver rescales it) and d (read by name, unused by Weigh2_dust) are
assigned as the driver does.

The particles come from the existing fixture <case>.npz (not duplicated here): positions, particle_type, the neighbour
list nb_idx.  Its dust has one mass below the default crit_mass, a neutral f_un and ~1.7 km/s velocities:
every output would be zero.  So these are drawn, seeded:
    dust masses x U(0.5, 2), crit_mass = their median;
    dust f_un uniform over columns 7..14, rows normalised;  mu_array from the composition (code_running.py:162);
    velocities + N(0, 5e4 m/s);
    densities = critical_density 10^U(-53.5, -49.5): with ~1e50 atoms in a grain, losses on either side of the
    reference's limit of 1 atom;
    sizes = nb_h, the dust's x U(0.6, 1.2): nb_h IS the distance to a particle's K-th neighbour, so as committed a pair sits
    exactly on the edge of the support (s^2 - r^2 = 0 to rounding, a [wd > 0] no bound can decide); rescaled, pairs fall on
    both sides of the edge and none on it.
Stored: the drawn inputs, the two results, the constants, the versions.

Conditions on the fixture asserted here (conditions, not thresholds; change the seed if one fails), counted by the
restatement tests/dust_oracle.py on the same inputs: some element accepted, some rejected, some rejected although its
own loss is below the limit; every decision's margin at least 1e6 times the bound's relative size there (dust_oracle's
`slack`: the library then decides as the restatement does); the outputs finite; the inputs unmodified.

Usage:  python tests/golden/make_golden_dust.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import REF  # noqa: E402
from make_golden_cool import load_reference_repaired  # noqa: E402

CASES = [("sphere_dust_n2048_k40", 7)]


def pad_intf(nsc):
    zero = nsc.intf[0]
    assert zero.__name__ == "zero_function" and len(nsc.intf) == 14
    nsc.intf = tuple(nsc.intf) + (zero,) * (len(nsc.mu_specie) - len(nsc.intf))
    assert len(nsc.intf) == len(nsc.mu_specie)


def draw(g, nsc, seed):
    rs = np.random.RandomState(seed)
    pt = g["particle_type"]
    n = pt.shape[0]
    dust = pt == 2
    nd = int(dust.sum())
    mass = np.array(g["mass"], dtype=np.float64)
    mass[dust] *= rs.uniform(0.5, 2.0, nd)
    crit_mass = float(np.median(mass[dust]))
    f = np.array(g["f_un"], dtype=np.float64)
    fd = np.zeros((nd, f.shape[1]))
    fd[:, 7:15] = rs.uniform(0.0, 1.0, (nd, 8))
    f[dust] = fd / np.sum(fd, axis=1)[:, None]
    mu = np.sum(f * nsc.mu_specie, axis=1) / np.sum(f, axis=1)
    vel = np.array(g["velocities"], dtype=np.float64) + rs.normal(0.0, 5e4, (n, 3))
    dens = float(nsc.critical_density) * 10.0 ** rs.uniform(-53.5, -49.5, n)
    sizes = np.array(g["nb_h"], dtype=np.float64)
    sizes[dust] *= rs.uniform(0.6, 1.2, nd)
    return mass, crit_mass, f, mu, vel, dens, sizes


def make(nsc, case, seed):
    import dust_oracle
    g = dict(np.load(os.path.join(HERE, case + ".npz"), allow_pickle=False))
    pts, pt = g["points"], g["particle_type"]
    nb = g["nb_idx"].astype(np.int64)
    mass, crit_mass, f_un, mu, vel, dens, sizes = draw(g, nsc, seed)
    nsc.crit_mass = crit_mass
    nsc.d = float(g["loop_d"])
    args = (pts, vel, nb, mass, f_un, mu, sizes, dens, pt)
    keep = [a.copy() for a in args]
    with np.errstate(all="ignore"):
        fd, fr = nsc.supernova_destruction(*args)
    for a, b in zip(keep, args):
        assert np.array_equal(a, b), "the reference modified an input"
    fd, fr = (np.ascontiguousarray(np.asarray(a, dtype=np.float64)) for a in (fd, fr))
    assert fd.shape == f_un.shape and fr.shape == f_un.shape
    assert np.all(np.isfinite(fd)) and np.all(np.isfinite(fr)), "outputs not finite"
    o = dust_oracle.destruction(*args, crit_mass=crit_mass, critical_density=float(nsc.critical_density), amu=float(nsc.amu))
    c = o["counts"]
    out = dict(velocities=vel, mass=mass, f_un=f_un, mu_array=mu, densities=dens, sizes=sizes, crit_mass=np.float64(crit_mass),
               critical_density=np.float64(nsc.critical_density), const_amu=np.float64(nsc.amu), seed=np.int64(seed),
               frac_destruction=fd, frac_reuptake=fr)
    import scipy
    out["versions"] = np.array(["numpy " + np.__version__, "scipy " + scipy.__version__, "python " + sys.version.split()[0]])
    path = os.path.join(HERE, "dust_" + case + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("%s: %d pairs in contributing rows; %s; margins %s; slack %s; frac_destruction != 0 on %d, frac_reuptake != 0 on %d; "
          "restatement equal bit for bit: destruction %s, reuptake %s (worst relative difference %.3g); %d bytes"
          % (path, o["pairs"], c, o["margins"], o["slack"], int(np.count_nonzero(fd)), int(np.count_nonzero(fr)),
             np.array_equal(fd, o["frac_destruction"]), np.array_equal(fr, o["frac_reuptake"]),
             dust_oracle.worst_ratio(o["frac_reuptake"], fr, np.abs(fr)), size))
    assert size <= 1000000, "fixture over the size limit"
    assert c["accepted"] > 0 and c["rejected"] > 0 and c["rejected_by_accumulation"] > 0, "a regime is empty: change the seed"
    assert min(o["slack"].values()) >= 1e6, "a decision within reach of the bound: change the seed"


def main():
    if not os.path.exists(REF):
        print("reference not present: nothing to do")
        return 0
    nsc, _ = load_reference_repaired()
    pad_intf(nsc)
    for case, seed in CASES:
        make(nsc, case, seed)
    return 0


if __name__ == "__main__":
    sys.exit(main())
