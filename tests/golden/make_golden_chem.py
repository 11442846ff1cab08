#!/usr/bin/env python3
"""Generate tests/golden/chem_<case>.npz: the reference's chemisputtering_2 (nsc:1265-1416) on seeded inputs.

CONTAINER-ONLY TOOL, a no-op (exit 0 with a message) where the reference is absent.  It loads the reference the way
make_golden_cool does (an in-memory Python-2 -> Python-3 transform; no reference text is stored; the repairs that loader
applies touch rad_cooling alone).  The module globals d and dt are assigned as the driver does.

The particles come from the existing fixture <case>.npz (not duplicated here): positions, particle_type, T, the
neighbour list nb_idx, the smoothing length d (loop_d).  Its dust has a neutral composition and its gas no ions, no
He++ and no refractory species: nothing would be sputtered, taken up or clamped.  So these are drawn, seeded:
    dust f_un uniform over columns 7..14, rows normalised;
    gas f_un: shares of H+ (U(0, 0.05)), He+ (U(0, 0.01)), He++ (U(0, 0.01)) and of every refractory column 7..14
    (U(0, 1e-4) each) added, rows normalised; the refractory entries of every second gas row then set to 0 - a count
    of exactly 0 cannot give anything away, which is clamp 1;
    mu_array from the composition (code_running.py:162);
    sizes = nb_h, the dust's x U(0.6, 1.2) (as make_golden_dust does);
    dt = dt_0 x 1e6: grains grow by accretion (F_sput > 1) until the gas rows run out of a species, so that rows
    sharing a gas particle depend on one another's clamped losses several levels deep.
Stored: the drawn inputs, both results, d, dt, the constants and tables, the versions.

Conditions on the fixture asserted here (conditions, not thresholds; change the seed if one fails), counted by the
restatement tests/chem_oracle.py on the same inputs: clamp-1 events > 0; the round model needs >= 3 rounds and ends on the
sequential result bit for bit; every decision's margin at least 1e6 times the bound's size there (chem_oracle's `slack`:
the library then decides as the restatement does); the outputs finite; the inputs unmodified.

Usage:  python tests/golden/make_golden_chem.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import REF  # noqa: E402
from make_golden_cool import load_reference_repaired  # noqa: E402

CASES = [("sphere_dust_n2048_k40", 6)]
DT_FACTOR = 1e6


def draw(g, mu_specie, seed):
    rs = np.random.RandomState(seed)
    pt = g["particle_type"]
    dust, gas = pt == 2, pt == 0
    nd, ng = int(dust.sum()), int(gas.sum())
    f = np.array(g["f_un"], dtype=np.float64)
    fd = np.zeros((nd, f.shape[1]))
    fd[:, 7:15] = rs.uniform(0.0, 1.0, (nd, 8))
    f[dust] = fd / np.sum(fd, axis=1)[:, None]
    fg = f[gas]
    fg[:, 3] += rs.uniform(0.0, 0.05, ng); fg[:, 4] += rs.uniform(0.0, 0.01, ng); fg[:, 5] += rs.uniform(0.0, 0.01, ng)
    fg[:, 7:15] += rs.uniform(0.0, 1e-4, (ng, 8))
    fg[::2, 7:15] = 0.0
    f[gas] = fg / np.sum(fg, axis=1)[:, None]
    mu = np.sum(f * mu_specie, axis=1) / np.sum(f, axis=1)
    sizes = np.array(g["nb_h"], dtype=np.float64)
    sizes[dust] *= rs.uniform(0.6, 1.2, nd)
    return f, mu, sizes


def make(nsc, case, seed):
    import chem_oracle
    g = dict(np.load(os.path.join(HERE, case + ".npz"), allow_pickle=False))
    pts, pt, T = g["points"], g["particle_type"], g["T"]
    mass = np.array(g["mass"], dtype=np.float64)
    nb = g["nb_idx"].astype(np.int64)
    f_un, mu, sizes = draw(g, nsc.mu_specie, seed)
    nsc.d = d = float(g["loop_d"])
    nsc.dt = dt = float(nsc.dt_0) * DT_FACTOR
    args = (pts, nb, mass, f_un, mu, sizes, T, pt)
    keep = [a.copy() for a in args]
    with np.errstate(all="ignore"), open(os.devnull, "w") as null:
        out_, sys.stdout = sys.stdout, null
        try:
            mass_new, f_new = nsc.chemisputtering_2(*args)
        finally:
            sys.stdout = out_
    for a, b in zip(keep, args):
        assert np.array_equal(a, b), "the reference modified an input"
    mass_new, f_new = (np.ascontiguousarray(np.asarray(a, dtype=np.float64)) for a in (mass_new, f_new))
    assert mass_new.shape == mass.shape and f_new.shape == f_un.shape
    assert np.all(np.isfinite(mass_new)) and np.all(np.isfinite(f_new)), "outputs not finite"
    consts = dict(k_B=float(nsc.k), amu=float(nsc.amu), m_0=float(nsc.m_0))
    o = chem_oracle.sputter(*args, d=d, dt=dt, model=True, mu_specie=nsc.mu_specie, mineral_densities=nsc.mineral_densities,
                            sputtering_yields=nsc.sputtering_yields, mrn=nsc.mrn_constants, **consts)
    c = o["counts"]
    out = dict(f_un=f_un, mu_array=mu, sizes=sizes, d=np.float64(d), dt=np.float64(dt), seed=np.int64(seed),
               mu_specie=np.asarray(nsc.mu_specie, dtype=np.float64), mineral_densities=np.asarray(nsc.mineral_densities, dtype=np.float64),
               sputtering_yields=np.asarray(nsc.sputtering_yields, dtype=np.float64), mrn=np.asarray(nsc.mrn_constants, dtype=np.float64),
               const_k=np.float64(nsc.k), const_amu=np.float64(nsc.amu), const_m_0=np.float64(nsc.m_0),
               mass_new=mass_new, f_un_new=f_new)
    import scipy
    out["versions"] = np.array(["numpy " + np.__version__, "scipy " + scipy.__version__, "python " + sys.version.split()[0]])
    path = os.path.join(HERE, "chem_" + case + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("%s: %s; slack %s; restatement equal bit for bit: mass_new %s, f_un_new %s; worst relative difference: mass_new %.3g, "
          "f_un_new %.3g; worst |diff| / bound: mass_new %.3g, f_un_new %.3g; %d bytes"
          % (path, c, o["slack"], np.array_equal(mass_new, o["mass_new"]), np.array_equal(f_new, o["f_un_new"]),
             chem_oracle.worst_ratio(o["mass_new"], mass_new, np.abs(mass_new)),
             chem_oracle.worst_ratio(o["f_un_new"], f_new, np.abs(f_new)),
             chem_oracle.worst_ratio(o["mass_new"], mass_new, o["mass_new_bound"]),
             chem_oracle.worst_ratio(o["f_un_new"], f_new, o["f_un_new_bound"]), size))
    assert size <= 1000000, "fixture over the size limit"
    assert c["clamp1"] > 0, "no clamp-1 event: change the seed"
    assert c["rounds"] >= 3, "no iteration needed: change the seed"
    assert min(o["slack"].values()) >= 1e6, "a decision within reach of the bound: change the seed"


def main():
    if not os.path.exists(REF):
        print("reference not present: nothing to do")
        return 0
    nsc, _ = load_reference_repaired()
    for case, seed in CASES:
        make(nsc, case, seed)
    return 0


if __name__ == "__main__":
    sys.exit(main())
