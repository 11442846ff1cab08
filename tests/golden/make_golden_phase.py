#!/usr/bin/env python3
"""Generate tests/golden/phase_a_<case>.npz and phase_b.npz: the dust phase of the reference DRIVER's time loop,
code_running.py:399-435, from the driver's own statements.

CONTAINER-ONLY TOOL, a no-op (exit 0 with a message) where the reference is absent.  The driver is a script that does
not run as a whole (make_golden_driver.py says why); the phase is one straight block of its loop.  This tool reads the
file at run time, takes the block BY LINE RANGE from the in-memory text - 399-427 and 430-435: line 428 is a Python-2
print statement that computes nothing kept - dedents it from the loop body and `exec`s it in a namespace that carries the
names it reads.  Only data is stored: what was put into the namespace and what the block left behind.  No source text.

Case (a): `nsc` is the reference module as make_golden_cool loads it (in memory, print statements transformed), with the
tuple of interpolants padded as make_golden_dust does (pad_intf).  The particles are the sphere of <case>.npz with the
dust fixture's masses, sizes, velocities and crit_mass and the chem fixture's composition, mu_array, d and dt = 1e6 dt_0
(none of it duplicated here).  mass and f_un go in as longdouble, as drv:153-155 leaves them.  Stored: every stage's
output.  The reference's guard compares an atom count with 1: on this set it rejects every loss and sputtering adds
exactly 0 (asserted) - the set pins the chain, the density and chemisputtering as the driver wires them.
Case (b): `nsc` is a stub whose stage functions return seeded arrays: NaNs in both fraction arrays, NaN entries in f_un
after chem, and destruction large enough to drive some masses negative - every regime of drv:412-433.  Stored: the stub's
arrays and what the block leaves.

Usage:  python tests/golden/make_golden_phase.py
"""
import contextlib
import io
import os
import sys
import textwrap

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden_driver import REF as DRIVER  # noqa: E402

CASE = "sphere_dust_n2048_k40"
KEPT = ("densities", "mass", "f_un", "mu_array", "gamma_array", "mass_reduction", "mass_increase", "mass_change", "delta_n",
        "prechems_mass")


def block(first, last):
    lines = open(DRIVER).read().split("\n")[first - 1:last]
    return compile(textwrap.dedent("\n".join(l.expandtabs(8) for l in lines)) + "\n", "code_running.py:%d-%d" % (first, last), "exec")


def driver_tables():
    """mu_specie, gamma, cross_sections, solar_mass, m_h as the driver assigns them: its block of physical constants and
    per-species tables, drv:25-57, taken by line range and executed as a whole like the phase itself (drv:58 adds a term of
    the reference module to cross_sections, which feeds only the optical depth the phase does not keep)."""
    import scipy.constants as constants
    ns = {"np": np, "constants": constants}
    exec(block(25, 57), ns)
    want = ("amu", "m_h", "solar_mass", "mu_specie", "cross_sections", "gamma")
    assert ns["mu_specie"].shape == ns["gamma"].shape == ns["cross_sections"].shape == (15,)
    return {w: ns[w] for w in want}


class Recorder(object):
    """Wraps the module the block calls: keeps what chemisputtering_2 and supernova_destruction return."""

    def __init__(self, mod):
        self._mod = mod
        self.kept = {}

    def __getattr__(self, name):
        fn = getattr(self._mod, name)
        if name not in ("chemisputtering_2", "supernova_destruction"):
            return fn

        def call(*a):
            res = fn(*a)
            self.kept[name] = tuple(np.array(r, dtype=np.float64) for r in res)
            return res
        return call


class Stub(object):
    """Case (b): the stage functions return seeded arrays."""

    def __init__(self, n, S, mass, mus, mu, seed):
        rs = np.random.RandomState(seed)
        self.dens = rs.uniform(0.5, 2.0, n) * 1e-18
        f = rs.uniform(0.0, 1.0, (n, S)); f[:, :2] += 3.0
        f /= f.sum(axis=1)[:, None]
        f[rs.rand(n, S) < 0.01] = np.nan
        self.f_chem = f.astype("longdouble")
        self.m_chem = (mass * (1.0 + 1e-3 * rs.normal(size=n))).astype("longdouble")
        destr = rs.uniform(0.0, 2e-3, (n, S)) * (rs.rand(n, S) < 0.5)
        reup = rs.uniform(0.0, 2e-3, (n, S)) * (rs.rand(n, S) < 0.5)
        heavy = rs.rand(n) < 0.08                       # rows that lose two to five times their mass
        scale = rs.uniform(2.0, 5.0, n) * mu / mus[9]
        destr[heavy, 9] = scale[heavy]
        destr[rs.rand(n, S) < 0.01] = np.nan
        reup[rs.rand(n, S) < 0.01] = np.nan
        self.destr, self.reup = destr, reup

    def density(self, *a):
        return self.dens.copy()

    def dust_density(self, *a):
        return self.dens.copy()

    def num_dens(self, *a):
        return self.dens.copy()

    def chemisputtering_2(self, *a):
        return self.m_chem.copy(), self.f_chem.copy()

    def supernova_destruction(self, *a):
        return self.destr.copy(), self.reup.copy()


def run(codes, ns):
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
        for c in codes:
            exec(c, ns)
    return {k_: np.array(ns[k_], dtype=np.float64) for k_ in KEPT}


def versions():
    import scipy
    return np.array(["numpy " + np.__version__, "scipy " + scipy.__version__, "python " + sys.version.split()[0]])


def main():
    if not os.path.exists(DRIVER):
        print("make_golden_phase: the reference is absent - nothing to do")
        return 0
    import chem_fixture
    import dust_fixture
    from make_golden_cool import load_reference_repaired
    from make_golden_dust import pad_intf
    codes = [block(399, 427), block(430, 435)]
    tab = driver_tables()
    base = dict(np=np, solar_mass=tab["solar_mass"], m_h=tab["m_h"], mu_specie=tab["mu_specie"], gamma=tab["gamma"],
                cross_sections=tab["cross_sections"])
    # ---- case (a) ----
    nsc, _ = load_reference_repaired()
    pad_intf(nsc)
    c, du = chem_fixture.load(), dust_fixture.load()
    assert np.array_equal(tab["mu_specie"], c["mu_specie"]) and np.array_equal(nsc.mu_specie, c["mu_specie"])
    nsc.d, nsc.dt, nsc.crit_mass = c["d"], c["dt"], du["crit_mass"]
    rec = Recorder(nsc)
    ns = dict(base, nsc=rec, points=c["points"].copy(), velocities=du["velocities"].copy(), neighbor=c["neighbor"].copy(),
              mass=du["mass"].astype("longdouble"), f_un=c["f_un"].astype("longdouble"), mu_array=c["mu_array"].copy(),
              sizes=du["sizes"].copy(), T=c["T"].copy(), particle_type=c["particle_type"].copy(), crit_mass=du["crit_mass"])
    res = run(codes, ns)
    m1, f1 = rec.kept["chemisputtering_2"]
    fd, fr = rec.kept["supernova_destruction"]
    assert not fd.any() and not fr.any(), "the reference's guard accepted a loss on this set: say so in the docstring"
    out = dict(density=res["densities"], mass_chem=m1, f_un_chem=f1, frac_destruction=fd, frac_reuptake=fr, mass=res["mass"],
               f_un=res["f_un"], mu_array=res["mu_array"], gamma_array=res["gamma_array"], gamma=tab["gamma"],
               totals=np.array([res["prechems_mass"], np.sum(m1), np.sum(res["mass"]), res["mass_reduction"], res["mass_increase"],
                                np.sum(res["mass_change"])]), crit_mass=np.float64(du["crit_mass"]), versions=versions())
    path = os.path.join(HERE, "phase_a_" + CASE + ".npz")
    np.savez_compressed(path, **out)
    moved = int(np.count_nonzero(np.abs(res["mass"] - du["mass"]) > 1e-6 * du["mass"]))
    print("%s: %d bytes; %d masses moved by more than 1e-6" % (path, os.path.getsize(path), moved))
    assert os.path.getsize(path) <= 1000000
    # ---- case (b) ----
    n, S, seed = 700, 15, 9107
    rs = np.random.RandomState(seed + 1)
    mass = 1e26 * (1.0 + rs.rand(n))
    mu = 1.0 + 50.0 * rs.rand(n)
    f0 = rs.uniform(0.0, 1.0, (n, S))
    crit_mass = float(np.median(mass))
    stub = Stub(n, S, mass, tab["mu_specie"], mu, seed)
    ns = dict(base, nsc=stub, points=None, velocities=None, neighbor=None, mass=mass.astype("longdouble"),
              f_un=f0.astype("longdouble"), mu_array=mu.copy(), sizes=None, T=None, particle_type=None, crit_mass=crit_mass)
    res = run(codes, ns)
    out = dict(in_mass=mass, in_f_un=f0, in_mu_array=mu, mass_chem=np.array(stub.m_chem, dtype=np.float64),
               f_un_chem=np.array(stub.f_chem, dtype=np.float64), frac_destruction=stub.destr, frac_reuptake=stub.reup,
               mass=res["mass"], f_un=res["f_un"], mu_array=res["mu_array"], gamma_array=res["gamma_array"], gamma=tab["gamma"],
               mu_specie=tab["mu_specie"],
               totals=np.array([res["prechems_mass"], np.sum(stub.m_chem), np.sum(res["mass"]), res["mass_reduction"],
                                res["mass_increase"], np.sum(res["mass_change"])], dtype=np.float64),
               crit_mass=np.float64(crit_mass), seed=np.int64(seed), versions=versions())
    path = os.path.join(HERE, "phase_b.npz")
    np.savez_compressed(path, **out)
    nreset = int(np.count_nonzero(res["mass"] == crit_mass / 200.))
    print("%s: %d bytes; %d masses reset, %d NaN entries in f_un after chem, %d / %d NaNs in the fractions"
          % (path, os.path.getsize(path), nreset, int(np.isnan(out["f_un_chem"]).sum()), int(np.isnan(stub.destr).sum()),
             int(np.isnan(stub.reup).sum())))
    assert os.path.getsize(path) <= 1000000
    assert nreset > 10 and np.isnan(out["f_un_chem"]).any() and np.isnan(stub.destr).any() and np.isnan(stub.reup).any()
    assert np.all(np.isfinite(res["mass"])) and np.all(np.isfinite(res["f_un"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
