#!/usr/bin/env python3
"""Generate tests/golden/sn_<case>.npz: the reference's supernova_impulse (nsc:1192-1204) on seeded inputs.

CONTAINER-ONLY TOOL, a no-op (exit 0 with a message) where the reference is absent.  It loads the reference the way
make_golden.load_reference does (an in-memory Python-2 -> Python-3 transform; no reference text is stored) and calls its
supernova_impulse as committed, once per star.

The particles come from the existing fixture <case>.npz (not duplicated here): positions and particle_type.  Its gas
masses would all be selected (the cloud weighs 1.2 solar masses, mass_displaced is 194.28), so the masses of the gas rows
are redrawn, seeded: m = U(0.5, 1.5) mass_displaced / 600 - about 600 of the 1943 gas rows reach the boundary.  The two
stars are the first two rows of type 1.

Stored: the drawn masses, the stars, per star the reference's d_vels and selected_points, the two module constants the
function reads, the versions.

Conditions on the fixture asserted here (conditions, not thresholds; change the seed if one fails), per star:
  0 < n_sel < n_gas;  the squared distances of the gas rows all distinct (so the reference's unstable argsort had no
  choice to make);  the star itself is no gas row.

Usage:  python tests/golden/make_golden_sn.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, load_reference  # noqa: E402

CASES = [("sphere_dust_n2048_k40", 7301)]


def make(nsc, case, seed):
    g = dict(np.load(os.path.join(HERE, case + ".npz"), allow_pickle=False))
    pts, pt = np.array(g["points"], dtype=np.float64), np.array(g["particle_type"], dtype=np.float64)
    rs = np.random.RandomState(seed)
    M = 194.28 * float(nsc.solar_mass)
    mass = np.array(g["mass"], dtype=np.float64)
    gas = pt == 0
    mass[gas] = rs.uniform(0.5, 1.5, int(gas.sum())) * M / 600.0
    stars = np.nonzero(pt == 1)[0][:2].astype(np.int64)
    assert stars.shape[0] == 2
    out = dict(mass=mass, stars=stars, const_solar_mass=np.float64(nsc.solar_mass),
               const_supernova_energy=np.float64(nsc.supernova_energy))
    keep = [a.copy() for a in (pts, mass, pt)]
    for t, ku in enumerate(stars):
        d_vels, sel = nsc.supernova_impulse(pts, mass, int(ku), pt)
        d_vels = np.ascontiguousarray(np.asarray(d_vels, dtype=np.float64))
        sel = np.asarray(sel, dtype=np.int64)
        s = np.sum((pts - pts[ku]) ** 2, axis=1)
        assert 0 < sel.shape[0] < int(gas.sum()), "the selection is not partial: change the draw"
        assert np.unique(s[gas]).shape[0] == int(gas.sum()), "two gas rows at the same distance: change the seed"
        assert not gas[ku]
        assert d_vels.shape == (sel.shape[0], 3) and np.all(np.isfinite(d_vels))
        out["d_vels_%d" % t] = d_vels
        out["selected_%d" % t] = sel
        print("star %d (row %d): %d of %d gas rows selected" % (t, ku, sel.shape[0], int(gas.sum())))
    for a, b in zip(keep, (pts, mass, pt)):
        assert np.array_equal(a, b), "the reference modified an input"
    import scipy
    out["versions"] = np.array(["numpy " + np.__version__, "scipy " + scipy.__version__, "python " + sys.version.split()[0]])
    path = os.path.join(HERE, "sn_" + case + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("%s: %d bytes" % (path, size))
    assert size <= 1000000, "fixture over the size limit"


def main():
    if not os.path.exists(REF):
        print("reference not present: nothing to do")
        return 0
    nsc = load_reference(False)
    for case, seed in CASES:
        make(nsc, case, seed)
    return 0


if __name__ == "__main__":
    sys.exit(main())
