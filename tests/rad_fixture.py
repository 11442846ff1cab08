"""The rad_<case>.npz fixtures joined with the particle fixtures they were made from, and rad_oracle's results on them,
computed once per (case, mode) and shared by the CPU and GPU tests (treat what comes back as read-only)."""
import functools
import os

import numpy as np

import rad_oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("sphere_dust_n2048_k40", "condensed_n1024_k40")
MIN_MARGIN = 1e-9


@functools.lru_cache(maxsize=None)
def load(case):
    """-> dict: positions, sizes, mu_array (the particle fixture), ptypes, masses, cross_array, sources, luminosities,
    targets, dt and the constants (the rad fixture), ref_<name> = the reference's captured results."""
    g = np.load(os.path.join(GOLDEN, case + ".npz"), allow_pickle=False)
    r = np.load(os.path.join(GOLDEN, "rad_" + case + ".npz"), allow_pickle=False)
    out = dict(positions=g["points"], sizes=g["nb_h"], mu_array=g["mu_array"], ptypes=r["particle_type"], masses=r["mass"],
               cross_array=r["cross_array"], sources=r["rs2"], luminosities=r["luminosities"], targets=r["rg2"],
               dt=float(r["dt"]), amu=float(r["const_amu"]), solar_luminosity=float(r["const_solar_luminosity"]),
               c=float(r["const_c"]), W6_constant=float(r["const_W6_constant"]))
    for nm in rad_oracle.OUTPUTS:
        out["ref_" + nm] = r[nm]
    return out


def transfer_args(f):
    """Positional arguments of compat.rad_transfer / rad_oracle.transfer."""
    return (f["positions"], f["ptypes"], f["masses"], f["sizes"], f["cross_array"], f["mu_array"], f["sources"],
            f["luminosities"], f["targets"], f["dt"])


def constants(f):
    return dict(amu=f["amu"], solar_luminosity=f["solar_luminosity"], c=f["c"])


@functools.lru_cache(maxsize=None)
def oracle(case, mode):
    f = load(case)
    return rad_oracle.transfer(*transfer_args(f), mode=mode, **constants(f))
