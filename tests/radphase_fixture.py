"""The radphase_*.npz fixtures (tests/golden/make_golden_radphase.py) joined with the particle, rad and cool fixtures they
were made from, as the arguments of the three array calls stage by stage - each stage fed the reference's own previous
outputs - and radphase_oracle's results on them, computed once and shared by the CPU and GPU tests (read-only)."""
import functools
import os

import numpy as np

import cool_fixture
import rad_fixture
import radphase_oracle as ro

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASE = "sphere_dust_n2048_k40"
SEED = 5101                                     # make_golden_rad.CASES[0]: the seed of the reference's own selection
STAGES = ("ionise", "heat", "cool")
HEAT_OUT = ("mu_array", "gamma_array", "cross_array", "E_internal", "T")
COOL_OUT = HEAT_OUT + ("velocities",)


def _npz(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))


@functools.lru_cache(maxsize=None)
def load(case):
    """case "a" or "b" -> dict: the block's inputs (particle_type, mass, mu_array, sizes, T, E_internal, velocities, f_un
    where the case has one), rad_heating's results rh_*, what the heating's bookkeeping left (heat_*), rad_cooling's
    results (cool_final_comp, cool_energy), what the block left (end_*), the constants, tables and scalars."""
    if case == "b":
        g = _npz("radphase_b")
        g["nsc_cross_sections"] = None
        return g
    g = _npz("radphase_a_" + CASE)
    g.update(_npz("radphase_a_cool_" + CASE))
    r, c = rad_fixture.load(CASE), cool_fixture.load(CASE)
    g.update(particle_type=r["ptypes"], mass=r["masses"], sizes=r["sizes"], points=r["positions"], f_un=c["f_un"], mu_array=c["mu_array"],
             T=c["T"], neighbor=c["neighbor"], d=c["d"], mu_specie=np.array(_mu_specie()))
    return g


def _mu_specie():
    import sph_code_amd.compat as nsc
    return nsc.mu_specie


def constants(g):
    return dict(t_cmb=float(g["const_t_cmb"]), t_max=float(g["t_max"]), k=float(g["const_k"]), m_h=float(g["const_m_h"]))


def photons_per_joule(g):
    """The scalar of nsc:976 for case (a)'s stars (compat.stellar_spectrum; tests/test_radphase_cpu.py holds it to the
    captured n_photons)."""
    import sph_code_amd.compat as nsc
    return nsc.stellar_spectrum(g["mass"][g["particle_type"] == 1])[1]


def ionise_args(g):
    """(f_un, ptypes, masses, lf2, frac_dest, photons_per_joule) and the tables (mu_specie, cross_sections, amu); case (a)."""
    return ((g["f_un"], g["particle_type"], g["mass"], g["rh_lf2"], g["rh_frac_dest"], photons_per_joule(g)),
            (g["mu_specie"], g["nsc_cross_sections"], float(g["const_amu"])))


def heat_args(g):
    """(f_un, ptypes, masses, mu_before, E_internal, T, lf2) - f_un is rad_heating's own."""
    return (g["rh_new_fun2"], g["particle_type"], g["mass"], g["mu_array"], g["E_internal"], g["T"], g["rh_lf2"])


def cool_args(g):
    """(final_comp, energy, ptypes, masses, sizes, E_internal, T, velocities, lf2, momentum) - E_internal and T are what the
    reference's heating left."""
    return (g["cool_final_comp"], g["cool_energy"], g["particle_type"], g["mass"], g["sizes"], g["heat_E_internal"], g["heat_T"],
            g["velocities"], g["rh_lf2"], g["rh_momentum"])


def tables(g):
    return (g["mu_specie"], g["gamma"], g["driver_cross_sections"])


@functools.lru_cache(maxsize=None)
def oracle(case, stage):
    g = load(case)
    c = constants(g)
    if stage == "ionise":
        a, t = ionise_args(g)
        return ro.ionise(*a, *t)
    if stage == "heat":
        return ro.heat_bookkeeping(*heat_args(g), *tables(g), c["t_cmb"], c["t_max"], c["k"], c["m_h"])
    return ro.cool_bookkeeping(*cool_args(g), *tables(g), float(g["dt"]), c["t_cmb"], c["t_max"], float(g["cooling_timescale"]),
                               float(g["const_sb"]), c["k"], c["m_h"])


def reference(case, stage):
    """The reference's own outputs of a stage, by the oracle's names."""
    g = load(case)
    if stage == "ionise":
        return dict(f_un_new=g["rh_new_fun2"], frac_destroyed=g["rh_frac_destroyed"])
    if stage == "heat":
        return {nm: g["heat_" + nm] for nm in HEAT_OUT}
    return {nm: g["end_" + nm] for nm in COOL_OUT}
