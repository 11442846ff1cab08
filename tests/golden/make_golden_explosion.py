#!/usr/bin/env python3
"""Generate tests/golden/explosion_a_<case>.npz and explosion_b_<case>.npz: the reference's supernova_explosion
(nsc:820-882) on seeded inputs, and the driver's insertion block (drv:363-382, 393-394) replayed on its outputs.

CONTAINER-ONLY TOOL, a no-op (exit 0 with a message) where the reference is absent.  It loads the reference the way
make_golden.load_reference does (an in-memory Python-2 -> Python-3 transform; no reference text is stored).  As committed
the function raises for the 15 species of the state: int_supernova holds 14 entries.  The
reference's own zero_function (int_supernova[0]) is appended IN MEMORY - the reading compat.supernova_destruction takes for
the same table - and the length asserted.  nsc.d_0 is assigned as drv:70 does, np.random is seeded, and the function is
called as committed.

The particles come from the existing fixture <case>.npz (not duplicated here).  Its stars weigh 1e-3 solar masses, outside
what an explosion is for: the masses of the exploding stars are redrawn, seeded, in [8, 40] solar masses.
  a: one star (the first row of type 1): all 16 outputs.
  b: two stars (the first two): every output but dustvels - with two or more stars nsc:858-859 index with the stale
     `position`: every dust row gets the LAST star's velocity and their number is n_sn x dust_len[last] (stored as
     ref_dustvels_rows for the record).  compat.supernova_explosion gives each dust row its own star's velocity.
Then drv:363-382 and drv:393-394 are replayed in plain NumPy on the reference's outputs (b: with the dust velocities under
that rule - the driver's own np.concatenate would leave velocities and points of different lengths) and the resulting
state is stored: T, mu_array, gamma_array, sizes and star_ages whole (every row of them is formed again), of the other
arrays the star rows and the new rows (the test checks the old rows against the inputs).

Conditions on the fixture asserted here (conditions, not thresholds; change the seed if one fails): at least one dust row
per star; the inputs unmodified (the reference's gas_release is a copy: its in-place /= touches nothing of f_un).

Usage:  python tests/golden/make_golden_explosion.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, load_reference  # noqa: E402

CASE = "sphere_dust_n2048_k40"
SEEDS = {"a": (1, 9101), "b": (2, 9102)}            # stars, seed
FIELDS = ("dust_comps", "gas_comps", "star_comps", "dust_mass", "gas_mass", "stars_mass", "newpoints", "newvels", "newgastype",
          "newdusttype", "new_eint_stars", "new_eint_dust", "new_eint_gas", "supernova_pos", "dustpoints", "dustvels")


def replay(nsc, g, mass, sp, out, star_ages, sizes, d, t_cmb):
    """drv:363-382, 393-394 with the driver's statements."""
    (dust_comps, gas_comps, star_comps, dust_mass, gas_mass, stars_mass, newpoints, newvels, newgastype, newdusttype, new_eint_stars,
     new_eint_dust, new_eint_gas, _, dustpoints, dustvels) = out
    particle_type = np.array(g["particle_type"], dtype=np.float64)
    E_internal, f_un, mass = np.array(g["E_internal"]), np.array(g["f_un"]), np.array(mass)
    velocities, points, T = np.array(g["velocities"]), np.array(g["points"]), np.array(g["T"])
    particle_type = np.concatenate((particle_type, newdusttype, newgastype))
    E_internal[sp] = new_eint_stars
    f_un[sp] = star_comps
    mass[sp] = stars_mass
    E_internal = np.concatenate((E_internal, new_eint_dust, new_eint_gas))
    mass = np.concatenate((mass, dust_mass, gas_mass))
    f_un = np.vstack([f_un, dust_comps, gas_comps])
    velocities = np.concatenate((velocities, dustvels, newvels))
    star_ages = np.concatenate((star_ages, np.ones(len(dustpoints)) * (-2), np.ones(len(sp)) * (-2)))
    points = np.vstack([points, dustpoints, newpoints])
    oldsizes = np.array(sizes)
    sizes = np.zeros(len(points))
    sizes[:len(oldsizes)] = oldsizes
    sizes[(particle_type == 0) & (sizes == 0)] = (mass[(particle_type == 0) & (sizes == 0)] / nsc.m_0) ** (1. / 3.) * d
    sizes[(particle_type == 1) & (sizes == 0)] = d / 10000.
    sizes[(particle_type == 2) & (sizes == 0)] = d
    Tnew = np.zeros(len(sizes))
    Tnew[:len(T)] += T
    T = Tnew
    T[T < t_cmb] = t_cmb
    mu_array = np.sum(f_un * nsc.mu_specie, axis=1) / np.sum(f_un, axis=1)
    gamma_array = np.sum(f_un * nsc.gamma, axis=1) / np.sum(f_un, axis=1)
    return dict(particle_type=particle_type, E_internal=E_internal, f_un=f_un, mass=mass, velocities=velocities, points=points,
                star_ages=star_ages, sizes=sizes, T=T, mu_array=mu_array, gamma_array=gamma_array)


def make(nsc, which):
    n_sn, seed = SEEDS[which]
    g = dict(np.load(os.path.join(HERE, CASE + ".npz"), allow_pickle=False))
    pt = np.array(g["particle_type"], dtype=np.float64)
    n = pt.shape[0]
    rs = np.random.RandomState(seed)
    sp = np.nonzero(pt == 1)[0][:n_sn].astype(np.int64)
    assert sp.shape[0] == n_sn
    mass = np.array(g["mass"], dtype=np.float64)
    mass[sp] = rs.uniform(8.0, 40.0, n_sn) * float(nsc.solar_mass)
    star_ages = np.where(pt == 1, rs.uniform(0.0, 1e14, n), -1.0)
    T = np.array(g["T"], dtype=np.float64)
    t_cmb = float(np.median(T))                     # (the reference's 2.732 K clamps no row of this cloud: half of them here)
    d = float(g["loop_d"])
    d_0 = float(np.median(g["nb_h"]))
    nsc.d_0 = d_0
    keep = [np.array(a) for a in (mass, g["points"], g["velocities"], g["E_internal"], g["f_un"])]
    np.random.seed(seed)
    out = nsc.supernova_explosion(mass, g["points"], g["velocities"], g["E_internal"], sp, g["f_un"])
    for a, b in zip(keep, (mass, g["points"], g["velocities"], g["E_internal"], g["f_un"])):
        assert np.array_equal(a, b), "the reference modified an input"
    out = [np.ascontiguousarray(np.asarray(a, dtype=np.float64)) if nm != "supernova_pos" else np.asarray(a, dtype=np.int64)
           for nm, a in zip(FIELDS, out)]
    n_dust = out[3].shape[0]
    assert out[14].shape == (n_dust, 3) and out[0].shape == (n_dust, 15)
    # the dust rows per star, as nsc:840-844 forms them from the outputs' own dust_comps: runs of equal rows
    assert n_sn <= 2
    dust_len = np.array([int(np.sum(np.all(out[0] == out[0][0 if t == 0 else -1], axis=1))) for t in range(n_sn)])
    assert dust_len.sum() == n_dust and np.all(dust_len >= 1), "a star without a dust row: change the seed"
    fix = dict(mass=mass, stars=sp, star_ages=star_ages, d=np.float64(d), d_0=np.float64(d_0), t_cmb=np.float64(t_cmb),
               seed=np.int64(seed), dust_len=dust_len, const_solar_mass=np.float64(nsc.solar_mass), const_m_0=np.float64(nsc.m_0))
    for nm, a in zip(FIELDS, out):
        if which == "b" and nm == "dustvels":
            fix["ref_dustvels_rows"] = np.int64(a.shape[0])
            assert a.shape[0] == n_sn * dust_len[-1] and np.all(a == g["velocities"][sp[-1]])
            continue
        fix["out_" + nm] = a
    if which == "b":                                # each dust row its own star's velocity
        out[15] = np.repeat(np.asarray(g["velocities"])[sp], dust_len, axis=0)
    st = replay(nsc, g, mass, sp, out, star_ages, g["nb_h"], d, t_cmb)
    assert st["points"].shape[0] == n + n_dust + n_sn == st["velocities"].shape[0]
    for key in ("T", "mu_array", "gamma_array", "sizes", "star_ages"):
        fix["state_" + key] = st[key]
    for key in ("particle_type", "E_internal", "f_un", "mass", "velocities", "points"):
        fix["state_star_" + key] = st[key][sp]
        fix["state_new_" + key] = st[key][n:]
    import scipy
    fix["versions"] = np.array(["numpy " + np.__version__, "scipy " + scipy.__version__, "python " + sys.version.split()[0]])
    path = os.path.join(HERE, "explosion_%s_%s.npz" % (which, CASE))
    np.savez_compressed(path, **fix)
    size = os.path.getsize(path)
    print("%s: %d stars, dust rows %s, %d bytes" % (path, n_sn, dust_len, size))
    assert size <= 1000000, "fixture over the size limit"


def main():
    if not os.path.exists(REF):
        print("reference not present: nothing to do")
        return 0
    nsc = load_reference(False)
    zero_function = nsc.int_supernova[0]
    assert zero_function.__name__ == "zero_function" and len(nsc.int_supernova) == 14
    nsc.int_supernova = tuple(nsc.int_supernova) + (zero_function,)
    assert len(nsc.int_supernova) == len(nsc.mu_specie) == 15
    for which in ("a", "b"):
        make(nsc, which)
    return 0


if __name__ == "__main__":
    sys.exit(main())
