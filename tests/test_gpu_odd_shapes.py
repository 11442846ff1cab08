"""GPU tests (-m gpu): odd N and K against the CPU oracle - the array API row by row (per-row bounds of
tests/oracle_bounds.py) and the fused step for three steps.  The shapes, and the oracle-only check that none of them is
vacuous, are in tests/test_odd_shapes_cpu.py.  These are ordinary small runs of supported shapes
(1 <= K <= SPHX_MAX_K, N >= 1, lists with missing entries where N <= K)."""
import numpy as np
import pytest

import oracle_bounds as ob
from test_odd_shapes_cpu import (ARRAY_CASES, STEP_CASES, case_id, case_state, hydro_modes, loop_with_drag, oracle_step,
                                 step_fixed_dt)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nsc():
    import sph_code_amd.compat as nsc_mod
    nsc_mod.context()
    return nsc_mod


@pytest.mark.parametrize("case", ARRAY_CASES, ids=case_id)
def test_array_api_vs_oracle_at_odd_shapes(nsc, case):
    """compat.neighbors -> compat.hydro_update (both visc_modes, clip_grad off and on) and the loop forms, every row
    against the oracle on the same arguments (the GPU's own idx, h; checked against SciPy's exact query first)."""
    from oracle import sph_oracle as orc
    workload, n, K = case
    s, d = case_state(workload, n, K)
    p, v = nsc.clamp_state(s["points"], s["velocities"])
    idx, _, dist, nontriv, h = nsc.neighbors(p, np.inf, K)
    oi, _, od, ont, oh = orc.neighbors(p, np.inf, K, eps=0.0)
    np.testing.assert_allclose(dist, od, rtol=2e-15, atol=0)
    assert (np.sort(idx, axis=1) == np.sort(oi, axis=1)).all() and np.array_equal(nontriv, ont)
    assert (nontriv == min(n, K)).all() and ((idx == n).any() == (n < K))            # missing entries: idx == N
    m, pt, mu, gam = s["mass"], s["particle_type"], s["mu_array"], s["gamma_array"]
    args = (idx, p, m, h, s["f_un"], pt, s["T"], mu, gam, v)
    for visc_mode, clip_grad in hydro_modes(K):
        out = nsc.hydro_update(*args, clip_grad=clip_grad, visc_mode=visc_mode)
        ref, scales = ob.hydro_reference(args, clip_grad=clip_grad, visc_mode=visc_mode)
        ob.compare_hydro(out, ref, scales, "%s %s clip=%d" % (case_id(case), visc_mode, clip_grad))
    nsc.d = d
    rho = nsc.density(p, m, pt, idx)
    f_un = s["f_un"] if loop_with_drag(K) else None
    ref = ob.loop_reference(p, v, m, pt, h, idx, d, s["E_internal"], s["T"], gam, mu, rho, f_un=f_un, workers=1)
    drag = ob.compare_loop(nsc, ref, p, v, m, pt, h, idx, d, s["E_internal"], s["T"], gam, mu, rho, case_id(case), f_un=f_un)
    if workload == "two_phase" and K >= 16:
        assert np.abs(drag[0]).max() > 0 and np.abs(drag[1]).max() > 0


@pytest.mark.parametrize("case", STEP_CASES, ids=case_id)
def test_fused_step_vs_oracle_at_odd_shapes(case):
    """Simulation.step for three steps against the oracle's step of the same mode, with the per-particle gates
    test_step_trajectory_vs_oracle applies at its third step (x to 1e-12 of the cloud size, v to 1e-10 of max|v|, dt rel
    1e-12) plus h and rho to rtol 1e-9.  No case needs a fixed Courant dt: the oracle keeps every one of these clouds finite
    and within ten cloud sizes for the three steps (test_step_sweep_case_is_not_vacuous)."""
    from sph_code_amd.sim import Simulation
    forms, workload, n, K = case
    s0, d = case_state(workload, n, K)
    fixed_dt = step_fixed_dt(case, s0)
    kw = dict(forms="loop", d=d, with_drag=(workload == "two_phase")) if forms == "loop" else \
        dict(visc_mode="pairwise" if forms == "pairwise" else "ref_axis0")
    sim = Simulation(s0, n_neigh=K, **kw)
    ref = dict(s0)
    for it in range(3):
        sim.step(1, fixed_dt=fixed_dt)
        ref = oracle_step(case, ref, d, it == 0, fixed_dt)
        got = sim.download()
        assert got["dt"] == pytest.approx(ref["dt"], rel=1e-12), "dt at step %d" % it
    R0 = np.max(np.abs(s0["points"]))
    for key in ("points", "velocities", "sizes", "densities"):
        assert np.isfinite(ref[key]).all() and np.isfinite(got[key]).all(), key
    ex = np.max(np.abs(got["points"] - ref["points"])) / R0
    ev = np.max(np.abs(got["velocities"] - ref["velocities"])) / np.max(np.abs(ref["velocities"]))
    print("%s: x err %.3g of the cloud size, v err %.3g of max|v|" % (case_id(case), ex, ev))
    assert ex <= 1e-12 and ev <= 1e-10
    np.testing.assert_allclose(got["sizes"], ref["sizes"], rtol=1e-9)
    np.testing.assert_allclose(got["densities"], ref["densities"], rtol=1e-9)
    assert np.any(got["total_accel"] != 0.0)
