"""One step of the CPU oracle in each of the step loop's modes (test helper, no test of its own): shared by the odd-shape
sweep (tests/test_odd_shapes_cpu.py, tests/test_gpu_odd_shapes.py) and the species sweep (tests/species_cases.py)."""
import numpy as np

from oracle import sph_oracle as orc


def oracle_step(case, ref, d, first, fixed_dt):
    """One step of the oracle in the case's mode."""
    forms, workload, n, K = case
    if forms == "loop":
        return orc.step_loop(ref, d, n_neigh=K, eps=0.0, first=first, fixed_dt=fixed_dt, with_drag=(workload == "two_phase"))
    if forms == "hydro_update":
        return orc.step(ref, n_neigh=K, eps=0.0, first=first, fixed_dt=fixed_dt)
    s = dict(ref)                                                                    # pairwise: orc.step's statements
    p, v = orc.clamp_state(s["points"], s["velocities"])
    nb, _, _, _, h = orc.neighbors(p, np.inf, K, eps=0.0)
    dt = fixed_dt if fixed_dt > 0 else orc.timestep(orc.crossing_time(nb, v, h, s["particle_type"]), first)
    with np.errstate(all="ignore"):
        ha, va, vh, rho, nden, _, _ = orc.hydro_update(nb, p, s["mass"], h, np.ones((len(p), 1)), s["particle_type"], s["T"],
                                                       s["mu_array"], s["gamma_array"], v, visc_mode="pairwise")
    p, v, total, E, T_ = orc.integrate(p, v, s["total_accel"], s["E_internal"], s["mass"], s["mu_array"], s["gamma_array"],
                                       s["particle_type"], ha, va, vh, dt)
    s.update(points=p, velocities=v, total_accel=total, E_internal=E, T=T_, dt=dt, sizes=h, densities=rho)
    return s
