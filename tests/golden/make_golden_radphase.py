#!/usr/bin/env python3
"""Generate tests/golden/radphase_a_<case>.npz, radphase_a_cool_<case>.npz and radphase_b.npz: the radiative block of the
reference DRIVER's time loop, code_running.py:247-316, from the driver's own statements.

CONTAINER-ONLY TOOL, a no-op (exit 0 with a message) where the reference is absent.  Like make_golden_phase.py it reads
the driver at run time, takes the block BY LINE RANGE from the in-memory text, dedents it and `exec`s it in a namespace
that carries the names it reads.  Only data is stored.  The driver never defines t_max and cooling_timescale (a NameError
as committed): they are put into the namespace, with N_RADIATIVE = 1 (drv:246), an empty supernova_pos (drv:244) and the
optical_depth the previous pass of the loop would have left (drv:250 reads it).

Case (a): `nsc` is the reference module as make_golden_cool loads it (np.minimum repairs), on the sphere of <case>.npz
with the six seeded stars, the masses and the seed of make_golden_rad.py (so the reference's own selection is that
fixture's), the cool fixture's ionised composition, mu_array and T, E_internal = N_PART gamma k T 10^U(-2, 0.5) and
dt = dt_0 / 1000 (at dt_0 the heating alone lifts every gas particle far above t_cmb: the lower clamp would stay empty).
Captured: rad_heating's frame locals (frac_dest, n_photons, frac_destroyed_by_species[:, :3], new_fun2 and the nine of
make_golden_rad.py), and what each stage of the block leaves: the namespace when rad_cooling is called (after the
heating's bookkeeping), rad_cooling's results, the namespace at the end.
Case (b): `nsc` is a stub whose rad_heating and rad_cooling return seeded arrays that drive every regime of the
bookkeeping: E_internal = 0 rows (inf -> DBL_MAX), negative E_internal (the exp branch of the first coefficient), NaN in
lf2, T below t_cmb and above t_max, energy large enough to underflow the exp.

Conditions asserted here (conditions, not thresholds: change the seed, not the threshold, when one fails): the column
margin above 1e-9; no atoms_total / amu in (0, 1e-9); both sides of each T clamp populated; E_change_coeff_0 >= 0 with
some > 0 and E_change_coeff_1 < 0 populated (the signs the block can produce on physical inputs); a dust particle with
lf2 > 0.

Usage:  python tests/golden/make_golden_radphase.py
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
from make_golden_rad import CAPTURE, MIN_MARGIN, call_capturing_locals  # noqa: E402

CASE, SEED = "sphere_dust_n2048_k40", 5101            # make_golden_rad.CASES[0]
T_MAX = 1e4
HEAT_KEPT = ("f_un", "mu_array", "gamma_array", "cross_array", "E_internal", "T")
END_KEPT = HEAT_KEPT + ("velocities",)
ION_LOCALS = ("frac_dest", "n_photons", "new_fun2")


def block(first, last):
    lines = open(DRIVER).read().split("\n")[first - 1:last]
    return compile(textwrap.dedent("\n".join(l.expandtabs(8) for l in lines)) + "\n", "code_running.py:%d-%d" % (first, last), "exec")


def driver_tables():
    """The driver's constants and per-species tables, drv:25-58 taken by line range (drv:58 adds sigma_effective)."""
    import scipy.constants as constants
    from make_golden import load_reference
    ns = {"np": np, "constants": constants, "nsc": load_reference(False)}
    exec(block(25, 58), ns)
    want = ("amu", "m_h", "k", "sb", "t_cmb", "solar_mass", "mu_specie", "cross_sections", "gamma")
    return {w: ns[w] for w in want}


class Recorder(object):
    """Wraps the module the block calls: rad_heating's locals; the namespace as it stands when rad_cooling is called and
    what rad_cooling returns."""

    def __init__(self, mod, ns):
        self._mod, self._ns = mod, ns
        self.heat_locals, self.at_cooling, self.cooling = {}, {}, None

    def __getattr__(self, name):
        fn = getattr(self._mod, name)
        if name == "rad_heating":
            def call(*a):
                if hasattr(fn, "__code__"):
                    res, loc = call_capturing_locals(fn, *a)
                    self.heat_locals = loc
                    return res
                return fn(*a)
            return call
        if name == "rad_cooling":
            def call(*a):
                self.at_cooling = {k_: np.array(self._ns[k_], dtype=np.float64) for k_ in HEAT_KEPT}
                res = fn(*a)
                self.cooling = tuple(np.array(r, dtype=np.float64) for r in res)
                return res
            return call
        return fn


class Stub(object):
    """Case (b): seeded results for the two physics calls."""

    def __init__(self, n, S, pt, f0, seed):
        rs = np.random.RandomState(seed)
        g = int(np.count_nonzero(pt != 1))
        self.lf2 = 10.0 ** rs.uniform(20, 40, g)
        self.lf2[rs.rand(g) < 0.03] = np.nan
        self.lf2[rs.rand(g) < 0.05] = 0.0
        self.mom = rs.normal(size=(g, 3)) * 10.0
        f = f0 * rs.uniform(0.5, 1.5, f0.shape)
        self.f_heat = f / f.sum(axis=1)[:, None]
        f = self.f_heat * rs.uniform(0.8, 1.2, f0.shape)          # rad_cooling's rows do not sum to 1
        self.f_cool = f
        self.energy = 10.0 ** rs.uniform(-30, -18, n) * np.where(rs.rand(n) < 0.15, -1.0, 1.0)
        self.energy[rs.rand(n) < 0.1] = 1e-8                       # -energy N_PART / E far below the exp's underflow
        self.rec = np.zeros((S, n))

    def rad_heating(self, *a):
        return self.lf2.copy(), self.f_heat.copy(), self.mom.copy(), np.zeros(len(self.lf2))

    def rad_cooling(self, *a):
        return self.f_cool.copy(), self.energy.copy(), self.rec.copy()


def run(code, ns):
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
        exec(code, ns)
    return {k_: np.array(ns[k_], dtype=np.float64) for k_ in END_KEPT}


def versions():
    import scipy
    return np.array(["numpy " + np.__version__, "scipy " + scipy.__version__, "python " + sys.version.split()[0]])


def base_namespace(tab, dt, cooling_timescale):
    return dict(np=np, N_RADIATIVE=1, m_h=tab["m_h"], k=tab["k"], sb=tab["sb"], t_cmb=tab["t_cmb"], t_max=T_MAX,
                cooling_timescale=cooling_timescale, solar_mass=tab["solar_mass"], mu_specie=tab["mu_specie"], gamma=tab["gamma"],
                cross_sections=tab["cross_sections"], dt=dt, supernova_pos=np.zeros(0, np.int64))


def stage_outputs(rec, end, prefix_heat="heat_", prefix_end="end_"):
    out = {prefix_heat + k_: v for k_, v in rec.at_cooling.items()}
    out.update({prefix_end + k_: v for k_, v in end.items()})
    out["cool_final_comp"], out["cool_energy"] = rec.cooling[0], rec.cooling[1]
    return out


def coefficients(lf2, E0, E1, energy, mass, mu_end, pt, m_h):
    """The two coefficients' quotients as the block forms them (for the generator's conditions only)."""
    gas_of_nonstar = pt[pt != 1] == 0
    with np.errstate(all="ignore"):
        c0 = np.nan_to_num(lf2[gas_of_nonstar] / E0[pt == 0])
        c1 = np.nan_to_num(-(energy * (mass / (m_h * mu_end)))[pt == 0] / E1[pt == 0])
    return c0, c1


def save(name, out):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("%s: %d bytes" % (path, size))
    assert size <= 1000000, "fixture over the size limit"


def main():
    if not os.path.exists(DRIVER):
        print("make_golden_radphase: the reference is absent - nothing to do")
        return 0
    import cool_fixture
    import rad_fixture
    import rad_oracle
    from make_golden_cool import load_reference_repaired
    code = block(247, 316)
    tab = driver_tables()
    # ---- case (a) ----
    nsc, _ = load_reference_repaired()
    r, c = rad_fixture.load(CASE), cool_fixture.load(CASE)
    assert np.array_equal(tab["mu_specie"], nsc.mu_specie)
    nsc.d = c["d"]
    pts, sizes, pt, mass = r["positions"], r["sizes"], r["ptypes"], r["masses"]
    n = len(mass)
    dt = 1e-3 * float(nsc.dt_0)                      # (at dt_0 the heating alone lifts every gas particle above 400 K)
    f_un, mu, T0 = c["f_un"].copy(), c["mu_array"].copy(), c["T"].copy()
    rs = np.random.RandomState(SEED + 7)
    gam0 = np.sum(f_un * tab["gamma"], axis=1) / np.sum(f_un, axis=1)
    cross0 = np.sum(f_un * tab["cross_sections"], axis=1) / np.sum(f_un, axis=1)
    E0 = mass / (tab["m_h"] * mu) * gam0 * tab["k"] * T0 * 10.0 ** rs.uniform(-2.0, 0.5, n)
    vel0 = rs.normal(size=(n, 3)) * 1e3
    cooling_timescale = 4.0 * dt
    ns = dict(base_namespace(tab, dt, cooling_timescale), points=pts.copy(), particle_type=pt.copy(), mass=mass.copy(), sizes=sizes.copy(),
              cross_array=cross0.copy(), f_un=f_un.copy(), mu_array=mu.copy(), T=T0.copy(), E_internal=E0.copy(),
              velocities=vel0.copy(), neighbor=c["neighbor"].copy(), optical_depth=mass / (tab["m_h"] * mu) * cross0)
    rec = Recorder(nsc, ns)
    ns["nsc"] = rec
    np.random.seed(SEED)
    end = run(code, ns)
    loc = rec.heat_locals
    for nm in ("rs2", "rg2", "luminosities"):
        assert np.array_equal(np.asarray(loc[nm], dtype=np.float64), r[{"rs2": "sources", "rg2": "targets"}.get(nm, nm)]), nm
    margin = min(rad_oracle.columns(pts, sizes, mass, mu, cross0, loc["rs2"], loc["rg2"], mode=m_, amu=float(nsc.amu))["margin"]
                 for m_ in rad_oracle.MODES)
    assert margin > MIN_MARGIN, "a (particle, ray) pair sits on a column's edge: change the seed, not the threshold"
    heat = dict(E_internal=E0, velocities=vel0, cross_array=cross0, t_max=np.float64(T_MAX), cooling_timescale=np.float64(cooling_timescale),
                dt=np.float64(dt), versions=versions())
    for nm in CAPTURE + ION_LOCALS:
        heat["rh_" + nm] = np.ascontiguousarray(np.asarray(loc[nm], dtype=np.float64))
    heat["rh_new_fun2"] = np.ascontiguousarray(heat["rh_new_fun2"].T)                      # (N,S), as returned
    heat["rh_frac_destroyed"] = np.ascontiguousarray(np.asarray(loc["frac_destroyed_by_species"], dtype=np.float64)[:, :3])
    for nm in ("k", "m_h", "amu", "sb", "t_cmb"):
        heat["const_" + nm] = np.float64(tab[nm])
    heat["gamma"], heat["driver_cross_sections"], heat["nsc_cross_sections"] = tab["gamma"], tab["cross_sections"], nsc.cross_sections
    heat["destruction_energies"] = np.asarray(nsc.destruction_energies, dtype=np.float64)
    stages = stage_outputs(rec, end)
    heat.update({k_: v for k_, v in stages.items() if k_.startswith("heat_")})
    cool = {k_: v for k_, v in stages.items() if not k_.startswith("heat_")}
    assert np.array_equal(stages["heat_f_un"], heat["rh_new_fun2"])
    del heat["heat_f_un"]                                                                   # (it is rh_new_fun2)
    assert np.array_equal(cool["end_f_un"], cool["cool_final_comp"])
    del cool["end_f_un"]
    save("radphase_a_" + CASE, heat)
    save("radphase_a_cool_" + CASE, cool)
    # the conditions
    at = np.asarray(loc["atoms_total"], dtype=np.float64) / float(nsc.amu)
    assert not np.any((at > 0) & (at < 1e-9)), "an atoms_total / amu inside (0, 1e-9): change the seed, not the threshold"
    lf2 = heat["rh_lf2"]
    c0, c1 = coefficients(lf2, E0, stages["heat_E_internal"], cool["cool_energy"], mass, end["mu_array"], pt, tab["m_h"])
    T1, T2 = stages["heat_T"], end["T"]
    fig = dict(margin=margin, c0_pos=int(np.sum(c0 > 0)), c0_neg=int(np.sum(c0 < 0)), c1_neg=int(np.sum(c1 < 0)), c1_pos=int(np.sum(c1 > 0)),
               T_heat_lo=int(np.sum(T1 == tab["t_cmb"])), T_heat_hi=int(np.sum(T1 == T_MAX)), T_heat_in=int(np.sum((T1 > tab["t_cmb"]) & (T1 < T_MAX))),
               T_end_lo=int(np.sum(T2 == tab["t_cmb"])), T_end_hi=int(np.sum(T2 == T_MAX)), T_end_in=int(np.sum((T2 > tab["t_cmb"]) & (T2 < T_MAX))),
               dust_lit=int(np.sum(lf2[pt[pt != 1] == 2] > 0)), frac_max=float(heat["rh_frac_destroyed"].max()))
    print("case (a):", fig)
    assert fig["c0_pos"] > 0 and fig["c1_neg"] > 0, "a coefficient's sign is not populated: change the seed, not the threshold"
    assert min(fig["T_heat_lo"], fig["T_heat_hi"], fig["T_heat_in"], fig["T_end_lo"], fig["T_end_hi"], fig["T_end_in"]) > 0, \
        "one side of a T clamp is empty: change the seed, not the threshold"
    assert fig["dust_lit"] > 0, "no dust particle with lf2 > 0: change the seed, not the threshold"
    # ---- case (b) ----
    n, S, seed = 700, 15, 9207
    rs = np.random.RandomState(seed + 1)
    pt = np.zeros(n)
    u = rs.rand(n)
    pt[u < 0.2] = 2.0
    pt[(u >= 0.2) & (u < 0.25)] = 1.0
    mass = 1e30 * (1.0 + rs.rand(n))
    f0 = rs.uniform(0.0, 1.0, (n, S)); f0[:, :3] += 2.0
    f0 /= f0.sum(axis=1)[:, None]
    mu = np.sum(f0 * tab["mu_specie"], axis=1) * rs.uniform(0.9, 1.1, n)
    sizes = 1e14 * (1.0 + rs.rand(n))
    T0 = 10.0 ** rs.uniform(-1.0, 6.0, n)
    E0 = mass / (tab["m_h"] * mu) * 1.6 * tab["k"] * 10.0 ** rs.uniform(-1.0, 6.0, n)
    E0[rs.rand(n) < 0.05] = 0.0
    E0[rs.rand(n) < 0.05] *= -1.0
    vel0 = rs.normal(size=(n, 3)) * 1e3
    dt = 7.9e12
    stub = Stub(n, S, pt, f0, seed)
    ns = dict(base_namespace(tab, dt, 2.0 * dt), points=None, particle_type=pt.copy(), mass=mass.copy(), sizes=sizes.copy(),
              cross_array=np.ones(n), f_un=f0.copy(), mu_array=mu.copy(), T=T0.copy(), E_internal=E0.copy(), velocities=vel0.copy(),
              neighbor=None, optical_depth=np.ones(n))
    rec = Recorder(stub, ns)
    ns["nsc"] = rec
    end = run(code, ns)
    out = dict(particle_type=pt, mass=mass, mu_array=mu, sizes=sizes, T=T0, E_internal=E0, velocities=vel0, dt=np.float64(dt),
               t_max=np.float64(T_MAX), cooling_timescale=np.float64(2.0 * dt), rh_lf2=stub.lf2, rh_momentum=stub.mom, rh_new_fun2=stub.f_heat,
               gamma=tab["gamma"], driver_cross_sections=tab["cross_sections"], mu_specie=tab["mu_specie"], seed=np.int64(seed),
               versions=versions())
    for nm in ("k", "m_h", "amu", "sb", "t_cmb"):
        out["const_" + nm] = np.float64(tab[nm])
    stages = stage_outputs(rec, end)
    del stages["heat_f_un"], stages["end_f_un"]
    out.update(stages)
    save("radphase_b", out)
    c0, c1 = coefficients(stub.lf2, E0, stages["heat_E_internal"], stub.energy, mass, end["mu_array"], pt, tab["m_h"])
    dmax = np.finfo(np.float64).max
    fig = dict(c0_dmax=int(np.sum(np.abs(c0) == dmax)), c0_neg=int(np.sum(c0 < 0)), c0_pos=int(np.sum(c0 > 0)), lf2_nan=int(np.isnan(stub.lf2).sum()),
               c1_under=int(np.sum(c1 < -746)), c1_pos=int(np.sum(c1 > 0)), T_lo=int(np.sum(end["T"] == tab["t_cmb"])),
               T_hi=int(np.sum(end["T"] == T_MAX)), T_heat_lo=int(np.sum(stages["heat_T"] == tab["t_cmb"])),
               T_heat_hi=int(np.sum(stages["heat_T"] == T_MAX)), E_nan=int(np.isnan(end["E_internal"]).sum()))
    print("case (b):", fig)
    assert min(fig["c0_dmax"], fig["c0_neg"], fig["c0_pos"], fig["lf2_nan"], fig["c1_under"], fig["c1_pos"], fig["T_lo"], fig["T_hi"],
               fig["T_heat_lo"], fig["T_heat_hi"]) > 0, "a regime of the bookkeeping is empty: change the seed, not the threshold"
    return 0


if __name__ == "__main__":
    sys.exit(main())
