#!/usr/bin/env python3
"""Generate tests/golden/rad_<case>.npz: the reference's rad_heating (nsc:893-1017) on seeded inputs, its locals captured.

CONTAINER-ONLY TOOL, a no-op (exit 0 with a message) where the reference is absent.  It loads the reference through
make_golden.load_reference (an in-memory transform; no reference text is stored) and calls its own rad_heating.  The
particles come from the existing fixtures <case>.npz (not duplicated here): positions, sizes = nb_h, mu_array, T, f_un.

Per case: six seeded particles are retyped as stars of (1, 3, 8, 20, 40, 0.5) solar masses beside whatever stars the
case has; cross_array = 10^U(-25, -21); np.random is seeded before the call, so the reference's own star selection
(nsc:901) and gas sampling (nsc:917) are reproducible.  The locals of rad_heating's frame are taken at its return
(sys.setprofile), as SURVEY 8c does for hydro_update.  Stored: the retyped particle_type and mass, cross_array, the
selected sources rs2, their luminosities, the sampled targets rg2, dt, the six results of nsc:922-965 (blocked,
star_distance, lum_factor, lf2, momentum, extinction), the constants they were formed with, and the versions.

The column is a top-hat: a particle whose distance to a ray's line is within rounding of its own h belongs to either
side.  The fixture is only valid where no (particle, ray) pair is that close: the smallest |d^2/h^2 - 1| (and, for
the segment reading, the two end tests) must exceed 1e-9 - if it does not, change the seed, not the threshold.

Usage:  python tests/golden/make_golden_rad.py
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import REF, SOLAR, load_reference  # noqa: E402

CASES = [("sphere_dust_n2048_k40", 5101), ("condensed_n1024_k40", 5102)]
STAR_MASSES = (1.0, 3.0, 8.0, 20.0, 40.0, 0.5)
CAPTURE = ("rs2", "rg2", "blocked", "star_distance", "luminosities", "lum_factor", "lf2", "momentum", "extinction")
MIN_MARGIN = 1e-9


def call_capturing_locals(fn, *args):
    """fn(*args) -> (result, the locals of fn's own frame at its return)."""
    code = fn.__code__
    box = {}

    def prof(frame, event, arg):
        if event == "return" and frame.f_code is code:
            box.update(frame.f_locals)

    sys.setprofile(prof)
    try:
        res = fn(*args)
    finally:
        sys.setprofile(None)
    return res, box


def make(nsc, case, seed):
    import rad_oracle
    g = dict(np.load(os.path.join(HERE, case + ".npz"), allow_pickle=False))
    pts, sizes, mu, T, f_un = g["points"], g["nb_h"], g["mu_array"], g["T"], g["f_un"]
    n = pts.shape[0]
    rs = np.random.RandomState(seed)
    ptype = g["particle_type"].copy()
    mass = g["mass"].copy()
    stars = rs.choice(np.nonzero(ptype == 0)[0], len(STAR_MASSES), replace=False)
    ptype[stars] = 1.0
    mass[stars] = np.array(STAR_MASSES) * SOLAR
    cross = 10.0 ** rs.uniform(-25.0, -21.0, n)
    dt = float(nsc.dt_0)
    np.random.seed(seed)
    sink = io.StringIO()                       # the reference prints every ray's index
    with contextlib.redirect_stdout(sink), np.errstate(all="ignore"):
        _, loc = call_capturing_locals(nsc.rad_heating, pts, ptype, mass, sizes, cross, f_un, np.zeros(0, np.int64), mu, T, dt)
    out = dict(particle_type=ptype, mass=mass, cross_array=cross, dt=np.float64(dt), stars=stars.astype(np.int64))
    for nm in CAPTURE:
        out[nm] = np.ascontiguousarray(np.asarray(loc[nm], dtype=np.float64))
    out["const_W6_constant"] = np.float64(nsc.W6_constant)
    out["const_amu"] = np.float64(nsc.amu)
    out["const_solar_luminosity"] = np.float64(nsc.solar_luminosity)
    out["const_c"] = np.float64(nsc.c)
    import scipy
    out["versions"] = np.array(["numpy " + np.__version__, "scipy " + scipy.__version__, "python " + sys.version.split()[0]])
    consts = dict(amu=float(nsc.amu), solar_luminosity=float(nsc.solar_luminosity), c=float(nsc.c))
    margins = {}
    for mode in rad_oracle.MODES:
        margins[mode] = rad_oracle.columns(pts, sizes, mass, mu, cross, out["rs2"], out["rg2"], mode=mode, **{"amu": consts["amu"]})["margin"]
    path = os.path.join(HERE, "rad_" + case + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("%s: %d sources x %d targets, margins %s, %d bytes" % (path, out["rs2"].shape[0], out["rg2"].shape[0], margins, size))
    assert size <= 1000000, "fixture over the size limit"
    assert min(margins.values()) > MIN_MARGIN, "a (particle, ray) pair sits on a column's edge: change the seed"


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
