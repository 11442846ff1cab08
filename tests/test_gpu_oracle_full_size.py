"""GPU tests (-m gpu): the array API against the CPU oracle on ALL rows at the timed size (10^6 particles, K = 40).

The full-size tests of tests/test_gpu_parity.py and tests/test_gpu_pairwise.py prove the timed step (LDS-form passes) equal
to the array API (gather kernels) at this size - HIP against HIP.  Here the array API itself meets the oracle at this size,
on the states those tests form (the state before step 1 and the state before step 2: clamped p, v; the GPU's own idx, h
from compat.neighbors, which test_full_size_properties pins against SciPy), every row, to the per-row bounds of
tests/oracle_bounds.py.  Together the two give the timed path an anchor outside the library.  Each test prints, per
output, the rows compared and the worst |x - ref| / (1e-12 sum_k|term_k|).
"""
import numpy as np
import pytest

import oracle_bounds as ob
from species_cases import live_composition

pytestmark = pytest.mark.gpu

N_FULL, K_FULL = 1_000_000, 40


@pytest.fixture(scope="module")
def nsc():
    import sph_code_amd.compat as nsc_mod
    nsc_mod.context()
    return nsc_mod


def _two_states(nsc, s, sim, fixed_dt=0.0):
    """The state before step 1 (the IC) and the state before step 2 (the fused loop's own, downloaded): clamped p, v, the
    temperature and energy of that instant."""
    p, v = nsc.clamp_state(s["points"], s["velocities"])
    yield "state 1", p, v, s["T"], s["E_internal"]
    sim.step(1, fixed_dt=fixed_dt)
    got = sim.download()
    p, v = nsc.clamp_state(got["points"], got["velocities"])
    yield "state 2", p, v, got["T"], got["E_internal"]


def _hydro_update_full_size(nsc, workload, visc_mode):
    import sph_code_amd.ics as ics
    from sph_code_amd.sim import Simulation
    n, K = N_FULL, K_FULL
    s = ics.WORKLOADS[workload](n)
    fixed_dt = ics.cfl_dt(s, K) if workload == "sedov" else 0.0
    sim = Simulation(s, n_neigh=K, visc_mode=visc_mode)
    fu1 = np.ones((n, 1))
    for label, p, v, T, _ in _two_states(nsc, s, sim, fixed_dt):
        label = "%s %s %s" % (workload, visc_mode, label)
        idx, _, _, nontriv, h = nsc.neighbors(p, np.inf, K)
        assert (nontriv == K).all()
        args = (idx, p, s["mass"], h, fu1, s["particle_type"], T, s["mu_array"], s["gamma_array"], v)
        out = nsc.hydro_update(*args, visc_mode=visc_mode)
        ref, scales = ob.hydro_reference(args, visc_mode=visc_mode)
        # the axis-0 viscosity is NaN on nearly every row from the second step on, by design (T < 0 after
        # step 1 -> sqrt of nsc:647): there the non-finite pattern must be the same and every finite row is compared
        nan_ok = visc_mode == "ref_axis0" and label.endswith("state 2")
        seen = ob.compare_hydro(out, ref, scales, label, visc_nonfinite_ok=nan_ok)
        if visc_mode == "ref_axis0" and not nan_ok:
            assert np.any(ref[1] != 0, axis=1).mean() > 0.9           # the viscous sums are live before step 1
        if visc_mode == "pairwise":
            assert np.any(ref[1] != 0, axis=1).mean() > 0.9 and (ref[2] >= 0).all()
        assert seen["density"] == n and seen["hydro_accel"] == n


@pytest.mark.timeout(600)
@pytest.mark.parametrize("workload", ["polytrope", "sedov"])
def test_hydro_update_vs_oracle_at_full_size(nsc, workload):
    """compat.hydro_update (ref_axis0): rho, rho_dust, n, F, hydro_accel, visc_accel, visc_heat against oracle.hydro_update,
    10^6 rows, both states (sedov under its fixed Courant dt, as test_timed_step_path_equals_array_path_at_full_size)."""
    _hydro_update_full_size(nsc, workload, "ref_axis0")


@pytest.mark.timeout(600)
def test_hydro_update_pairwise_vs_oracle_at_full_size(nsc):
    """compat.hydro_update(visc_mode="pairwise") against the oracle's pairwise restatement (pinned to the fixtures by
    tests/test_pairwise_cpu.py), 10^6 rows, both states; nothing non-finite in either."""
    _hydro_update_full_size(nsc, "polytrope", "pairwise")


def _loop_forms_full_size(nsc, workload, with_drag):
    import sph_code_amd.ics as ics
    from sph_code_amd.sim import Simulation
    n, K = N_FULL, K_FULL
    s = ics.WORKLOADS[workload](n)
    d = ics.loop_d(s, K)
    m, pt, mu, gam = s["mass"], s["particle_type"], s["mu_array"], s["gamma_array"]
    f_un = s["f_un"] if with_drag else None
    live = live_composition(s, 15, seed=N_FULL) if with_drag else None
    sim = Simulation(s, n_neigh=K, forms="loop", d=d, with_drag=with_drag)
    for label, p, v, T, E in _two_states(nsc, s, sim):
        label = "%s %s" % (workload, label)
        nsc.d = d
        idx, _, _, nontriv, h = nsc.neighbors(p, np.inf, K)
        assert (nontriv == K).all()
        rho = nsc.density(p, m, pt, idx)                  # the driver hands nsc.density's output on (drv:451,458)
        ref = ob.loop_reference(p, v, m, pt, h, idx, d, E, T, gam, mu, rho, f_un=f_un)
        drag = ob.compare_loop(nsc, ref, p, v, m, pt, h, idx, d, E, T, gam, mu, rho, label, f_un=f_un)
        assert np.any(ref["artificial_viscosity"][0] != 0, axis=1)[pt == 0].mean() > 0.9
        if with_drag:
            assert np.abs(drag[0]).max() > 0 and np.abs(drag[1]).max() > 0          # on the gas, and back on the dust
            assert np.abs(ref["net_impulse"][0]).max() > 0 and np.abs(ref["net_impulse"][1]).max() > 0
            # the species pass's array form: F (15 species, on a composition with every species > 0 and a row of its own
            # per particle: tests/species_cases.py) and the dust density of hydro_update
            args = (idx, p, m, h, live, pt, T, mu, gam, v)
            out = nsc.hydro_update(*args)
            href, scales = ob.hydro_reference(args)
            seen = ob.compare_hydro(out, href, scales, label + " hydro_update", which=(3, 4, 5, 6))
            assert seen["f_un_neighbor"] == n and (href[5][:2] > 0).any(axis=1).all() and (href[6] > 0).any()


@pytest.mark.timeout(600)
def test_loop_forms_vs_oracle_at_full_size(nsc):
    """Uniform cube (the reference's own IC): compat.density, dust_density, num_dens, del_pressure, artificial_viscosity
    and crossing_time against the oracle's loop forms, 10^6 rows, both states."""
    _loop_forms_full_size(nsc, "uniform_cube", False)


@pytest.mark.timeout(600)
def test_two_phase_loop_forms_drag_and_species_vs_oracle_at_full_size(nsc):
    """Two-phase cloud (10 % dust particles, 15 species): the loop forms, both returns of compat.net_impulse and
    hydro_update's F / dust density against the oracle, 10^6 rows, both states."""
    _loop_forms_full_size(nsc, "two_phase", True)
