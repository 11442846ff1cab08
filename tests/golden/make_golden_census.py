#!/usr/bin/env python3
"""Golden vectors for the census, the schedule and the run outputs from the reference DRIVER's own statements.

CONTAINER-ONLY TOOL (no-op when /root/reference is absent).  sph/code_running.py does not run as a whole
(make_golden_driver.py says why); the statements the census answers are straight-line code:

    code_running.py:244       supernova_pos
    code_running.py:339-341   max_rel_age, the largest stellar mass (printed)
    code_running.py:604       the stellar clock
    code_running.py:616-622   star_massfrac, star_numfrac, dust_temps and the histories of their length
    code_running.py:656-664   gas_, star_, dust_mass_by_species and the AGB_* arrays

This tool reads the file at run time, takes each range BY LINE RANGE from the in-memory text (tabs expanded, dedented) and
`exec`s them in that order in one namespace of seeded arrays.  nsc is the reference's own module through
make_golden.load_reference, as make_golden_explosion.py loads it.  What is stored is data only: the inputs put into the
namespace and the values the statements left behind.  No source text.

    census_a   n = 3000, S = 15; gas, stars and dust 70 / 10 / 20; stars on both sides of the 1-7 solar-mass window and
               of relative age 1
    census_b   n = 2048; no dust; one star exactly at star_ages == -2; one star whose relative age is the first double
               above 1 that its age can give, one the last below
"""
import contextlib
import io
import os
import sys
import textwrap

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import load_reference  # noqa: E402

REF = "/root/reference/sph/code_running.py"
RANGES = ((244, 244), (339, 341), (604, 604), (616, 622), (656, 664))
OUT_ARRAYS = ("supernova_pos", "gas_mass_by_species", "star_mass_by_species", "dust_mass_by_species", "AGB_condition", "AGB_list",
              "AGB_time_until", "AGB_metallicity", "AGB_composition", "dust_temps", "time_coord", "star_frac", "imf_measure")


def block(first, last):
    lines = open(REF).read().split("\n")[first - 1:last]
    return compile(textwrap.dedent("\n".join(l.expandtabs(8) for l in lines)) + "\n", "code_running.py:%d-%d" % (first, last), "exec")


def rel_age(nsc, ages, mass):
    """drv:244's left-hand side, for placing the near-1 stars (the fixture's results come from the exec'd statements)."""
    return ages / nsc.luminosity_relation(mass / nsc.solar_mass, np.ones(len(mass)), 1) / (nsc.year * 1e10)


def make_case(nsc, seed, n, probs, near_one):
    rng = np.random.RandomState(seed)
    S = len(nsc.mu_specie)
    particle_type = rng.choice([0., 1., 2.], size=n, p=probs)
    star = particle_type == 1
    mass = np.exp(rng.uniform(np.log(0.05), np.log(5.0), size=n)) * nsc.solar_mass
    mass[star] = np.exp(rng.uniform(np.log(0.3), np.log(30.0), size=np.count_nonzero(star))) * nsc.solar_mass
    f_un = rng.rand(n, S) * np.array([1.] * 2 + [0.05] * 5 + [0.01] * (S - 7)) + 1e-4
    f_un[particle_type == 2, :7] *= 1e-3
    T = np.exp(rng.uniform(np.log(3.), np.log(1e4), size=n))
    star_ages = -np.ones(n)
    life = nsc.luminosity_relation(mass / nsc.solar_mass, np.ones(n), 1) * 1e10 * nsc.year
    star_ages[star] = (life * rng.uniform(0., 2., size=n))[star]
    dusty = np.flatnonzero(particle_type == 2)
    star_ages[dusty[::5]] = -2.                                  # rows a supernova inserted (drv:371)
    dt = 2.5e5 * nsc.year * 0.37
    if near_one:
        stars = np.flatnonzero(star)
        frozen, above, below = stars[3], stars[10], stars[20]
        star_ages[frozen] = -2.                                  # a star the clock must leave alone
        for row, want_above in ((above, True), (below, False)):
            a = life[row]
            one = np.array([mass[row]])
            # the two roundings of the ratio can give exactly 1 over a few neighbouring ages: walk to the first age on
            # the wanted side of it
            if want_above:
                while not rel_age(nsc, np.array([a]), one)[0] > 1.:
                    a = np.nextafter(a, np.inf)
            else:
                while not rel_age(nsc, np.array([a]), one)[0] < 1.:
                    a = np.nextafter(a, -np.inf)
            star_ages[row] = a
        r = rel_age(nsc, star_ages[[above, below]], mass[[above, below]])
        print("near-1 relative ages:", repr(float(r[0])), repr(float(r[1])))
        assert 1. < r[0] <= 1. + 2. ** -52 and 1. - 2. ** -52 <= r[1] < 1., r.tolist()           # within 2^-52, the ulp of 1
    return dict(mass=mass, particle_type=particle_type, f_un=f_un, T=T, star_ages=star_ages, dt=np.float64(dt),
                age=np.float64(3.1e6 * nsc.year), OVERALL_AGE=np.float64(4.2e8 * nsc.year))


def run_blocks(nsc, codes, inp):
    ns = dict(np=np, nsc=nsc, solar_mass=nsc.solar_mass, year=nsc.year, mu_specie=np.array(nsc.mu_specie, dtype=np.float64),
              mass=inp["mass"].copy(), particle_type=inp["particle_type"].copy(), f_un=inp["f_un"].copy(), T=inp["T"].copy(),
              star_ages=inp["star_ages"].copy(), dt=float(inp["dt"]), age=float(inp["age"]), OVERALL_AGE=float(inp["OVERALL_AGE"]),
              time_coord=np.array([]), dust_temps=np.array([]), star_frac=np.array([]), imf_measure=np.array([]))
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
        for code in codes:
            exec(code, ns)
    out = {"out_" + k: np.asarray(ns[k]) for k in OUT_ARRAYS}
    out.update(out_max_rel_age=np.float64(ns["max_rel_age"]), out_star_ages=ns["star_ages"],
               out_star_massfrac=np.float64(ns["star_massfrac"]), out_star_numfrac=np.float64(ns["star_numfrac"]))
    for k in ("mass", "particle_type", "f_un", "T"):
        assert np.array_equal(ns[k], inp[k]), k                  # the statements modify star_ages alone
    return out


def main():
    if not os.path.exists(REF):
        print("reference not present: nothing to do")
        return
    nsc = load_reference(False)
    codes = [block(a, b) for a, b in RANGES]
    for name, seed, n, probs, near in (("census_a", 6161, 3000, [0.7, 0.1, 0.2], False), ("census_b", 6562, 2048, [0.85, 0.15, 0.0], True)):
        inp = make_case(nsc, seed, n, probs, near)
        out = run_blocks(nsc, codes, inp)
        np.savez_compressed(os.path.join(HERE, name + ".npz"), mu_specie=np.array(nsc.mu_specie, dtype=np.float64),
                            solar_mass=np.float64(nsc.solar_mass), year=np.float64(nsc.year), **inp, **out)
        print(name, "n", n, "supernovae", out["out_supernova_pos"].shape[0], "AGB", out["out_AGB_list"].shape[0], "dust",
              out["out_dust_temps"].shape[0], "max_rel_age", float(out["out_max_rel_age"]))


if __name__ == "__main__":
    main()
