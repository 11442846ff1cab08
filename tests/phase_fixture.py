"""The input sets of the dust-phase tests (tests/test_phase_cpu.py, tests/test_gpu_phase.py): states a Simulation can be
built from, each with the arguments of the phase (d, dt, the per-species tables, crit_mass) and the fixed step under
which the state is stepped once before the phase runs.  Built once per set and shared (treat what comes back as
read-only)."""
import functools
import os

import numpy as np

import chem_fixture
import chem_oracle
import dust_fixture
import dust_oracle
import phase_oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K_B = chem_oracle.K_B
M_H = 1.0008 * chem_oracle.AMU
STATE_KEYS = ("points", "velocities", "mass", "particle_type", "f_un", "T", "mu_array", "gamma_array", "E_internal", "total_accel")
MOVE_LIMIT = 0.01                # no particle moves further than this share of its h in the one step

# (n, K, S, seed): n around the 256-lane workgroup and beyond one (npad != n), K and S at every padded width (sp = 16, 16,
# 32), n = 33 < K = 40 (missing entries).  The seeds are chem_fixture's, which meet chem_oracle's margin condition.
SHAPES = ((257, 7, 15, 513), (257, 40, 15, 544), (257, 64, 15, 569), (2049, 7, 32, 517), (2049, 40, 32, 545), (257, 40, 7, 41),
          (33, 40, 15, 73))


def shape_id(spec):
    return "n=%d K=%d S=%d" % spec[:3]


def _complete(f, velocities, crit_mass):
    """The rest of a state around chemisputtering_2's arguments."""
    S = f["f_un"].shape[1]
    gam_t = phase_oracle.gamma_table(S)
    fun = f["f_un"]
    gam = np.sum(fun * gam_t, axis=1) / np.sum(fun, axis=1)                           # drv:163
    E = gam * f["mass"] * K_B * f["T"] / (f["mu_array"] * M_H)                        # drv:166
    n = len(f["mass"])
    out = dict(f, velocities=velocities, gamma_array=gam, E_internal=E, total_accel=np.zeros((n, 3)), gamma=gam_t,
               crit_mass=float(crit_mass), critical_density=dust_oracle.CRITICAL_DENSITY)
    # a step under which nothing moves further than half of MOVE_LIMIT h by its velocity (tests/test_phase_cpu.py checks the
    # whole move with the oracle's step)
    speed = np.sqrt(np.sum(velocities ** 2, axis=1))
    out["fixed_dt"] = float(0.5 * MOVE_LIMIT * np.min(f["sizes"] / np.maximum(speed, 1e-300)))
    return out


@functools.lru_cache(maxsize=None)
def state(n, K, S, seed):
    """chem_fixture.cloud plus velocities in dust_fixture.cloud's style, gamma_array and E_internal as the driver forms
    them, crit_mass = the median dust mass -> dict: the state (STATE_KEYS), neighbor and sizes (the cloud's own: the
    resident call takes the step's), d, dt, mu_specie, gamma, mineral_densities, sputtering_yields, crit_mass,
    critical_density, fixed_dt."""
    f = chem_fixture.cloud(n, K, S, seed)
    rs = np.random.RandomState(seed + 5000)
    vel = rs.normal(0.0, 7e4, (n, 3))
    isd = f["particle_type"] == 2.0
    m = f["mass"]
    return _complete(f, vel, np.median(m[isd]) if isd.any() else np.median(m))


@functools.lru_cache(maxsize=None)
def sphere():
    """The sphere of sphere_dust_n2048_k40 with the dust fixture's masses, velocities and crit_mass and the chem
    fixture's composition, d and dt = 1e6 dt_0 (with the chem fixture's own masses the dust stage is empty)."""
    c, du = chem_fixture.load(), dust_fixture.load()
    f = dict(points=c["points"], neighbor=c["neighbor"], mass=du["mass"], f_un=c["f_un"], mu_array=c["mu_array"], sizes=du["sizes"],
             T=c["T"], particle_type=c["particle_type"], d=c["d"], dt=c["dt"], mu_specie=c["mu_specie"],
             mineral_densities=c["mineral_densities"], sputtering_yields=c["sputtering_yields"])
    return _complete(f, du["velocities"], du["crit_mass"])


def sim_state(f):
    return {k_: f[k_] for k_ in STATE_KEYS}


def tables(f):
    """The table keywords of compat.dust_phase / Simulation.dust_phase."""
    return dict(mu_specie=f["mu_specie"], gamma=f["gamma"], mineral_densities=f["mineral_densities"],
                sputtering_yields=f["sputtering_yields"], crit_mass=f["crit_mass"], critical_density=f["critical_density"])


@functools.lru_cache(maxsize=None)
def load_golden(which):
    """-> tests/golden/phase_a_sphere_dust_n2048_k40.npz ("a": the reference's stages on sphere()) or phase_b.npz ("b":
    stub stages, the bookkeeping in every regime) as a dict (tests/golden/make_golden_phase.py)."""
    name = "phase_a_sphere_dust_n2048_k40.npz" if which == "a" else "phase_b.npz"
    return dict(np.load(os.path.join(GOLDEN, name), allow_pickle=False))
