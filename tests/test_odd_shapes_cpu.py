"""The shapes of the odd-N / odd-K sweep (tests/test_gpu_odd_shapes.py) and, oracle only, the check that none of them is
vacuous: on every (workload, N, K) the oracle's outputs are finite on every row the GPU test compares.

K in {1, 2, 7, 16, 33, 40, 63, 64} (SPHX_MAX_K = 64), N in {K + 1, 127, 128, 129, 1000, 4097, 8191, 8193, 20011} around the
128-particle blob and the 8192-element scan tile: every K with at least two ragged N, every N with K = 40 and an odd K, and
N <= K, where the lists carry missing entries (idx == N).  Also the six cases tools/odd_sizes_check.py used to run.

K = 1: the list is the particle itself, the kNN radius h = 0 and every sum of hydro_update is 0/0 - in the reference as
here; those shapes are compared through the loop forms with the global d (all but net_impulse, whose kernel width is h).
K = 2 on the two-phase cloud leaves dust rows without a gas neighbour (rho = 0, hydro_accel 0/0): the K = 2 shapes are gas
clouds.  (At K = 2 with clip_grad the pressure sum is exactly zero - the only neighbour sits on the edge of the own
kernel and outside the neighbour's - so "hydro_accel is live" is asked of the unclipped form.)
"""
import numpy as np
import pytest

from oracle import sph_oracle as orc
from step_oracle import oracle_step  # noqa: F401  (tests/test_gpu_odd_shapes.py takes it from here)

P, C, T = "polytrope", "uniform_cube", "two_phase"
ARRAY_CASES = [
    # every N with K = 40 ...
    (P, 41, 40), (C, 127, 40), (T, 128, 40), (P, 129, 40), (P, 1000, 40), (T, 4097, 40), (C, 8191, 40), (P, 8193, 40),
    (T, 20011, 40), (C, 1537, 40),
    # ... and with an odd K; N = K + 1 for every K
    (P, 2, 1), (C, 3, 2), (C, 8, 7), (T, 17, 16), (T, 34, 33), (P, 64, 63), (C, 65, 64),
    (T, 127, 7), (P, 128, 33), (C, 129, 63), (T, 1000, 33), (P, 4097, 7), (T, 8191, 63), (C, 8193, 33), (C, 20011, 7),
    # two ragged N and more for the remaining K
    (C, 777, 1), (P, 1000, 1), (C, 129, 2), (P, 8193, 2), (P, 100, 7), (C, 4097, 16), (P, 127, 16), (P, 5000, 64),
    (T, 8191, 64), (C, 1000, 64), (P, 1000, 63),
    # N <= K: lists with missing entries
    (C, 40, 64), (P, 5, 7), (T, 33, 40), (P, 16, 16),
]
# (forms, workload, N, K): hydro_update mode, pairwise mode, loop-form mode (two_phase: with drag)
STEP_CASES = [
    ("hydro_update", P, 129, 7), ("hydro_update", P, 1000, 33), ("hydro_update", P, 8193, 64), ("hydro_update", C, 40, 64),
    ("pairwise", P, 129, 33), ("pairwise", P, 1000, 64), ("pairwise", P, 8193, 7), ("pairwise", P, 5, 7),
    ("loop", C, 129, 64), ("loop", C, 1000, 7), ("loop", C, 8193, 33), ("loop", T, 1000, 33), ("loop", C, 40, 64),
]


def case_id(c):
    return "-".join(str(x) for x in c)


def case_state(workload, n, K):
    import sph_code_amd.ics as ics
    s = ics.WORKLOADS[workload](n)
    # the loop forms' global d from the 8th neighbour at least: at K = 1 the list's own radius is 0
    return s, ics.loop_d(s, min(max(K, 8), n))


def hydro_modes(K):
    """(visc_mode, clip_grad) pairs compared through hydro_update at this K."""
    return [] if K == 1 else [("ref_axis0", False), ("ref_axis0", True), ("pairwise", False), ("pairwise", True)]


def loop_with_drag(K):
    return K > 1


def _all_finite(x):
    return all(np.isfinite(np.asarray(a)).all() for a in (x if isinstance(x, tuple) else (x,)) if a is not None)


@pytest.mark.parametrize("case", ARRAY_CASES, ids=case_id)
def test_array_sweep_case_is_not_vacuous(case):
    workload, n, K = case
    s, d = case_state(workload, n, K)
    p, v = orc.clamp_state(s["points"], s["velocities"])
    idx, _, _, nontriv, h = orc.neighbors(p, np.inf, K, eps=0.0)
    assert (nontriv == min(n, K)).all() and ((idx == n).any() == (n < K))
    m, pt = s["mass"], s["particle_type"]
    args = (idx, p, m, h, s["f_un"], pt, s["T"], s["mu_array"], s["gamma_array"], v)
    for visc_mode, clip_grad in hydro_modes(K):
        with np.errstate(all="ignore"):
            out, inter = orc.hydro_update(*args, return_intermediates="rows", clip_grad=clip_grad, visc_mode=visc_mode)
        assert _all_finite(tuple(out)), (visc_mode, clip_grad, [np.isfinite(o).all() for o in out])
        assert all(np.isfinite(inter[k_]).all() for k_ in ("G_abs_terms", "visc_abs_terms", "visc_heat_abs_terms"))
        assert clip_grad or np.any(out[0] != 0)
    rho = orc.density(p, m, pt, idx, d)
    assert _all_finite(rho) and (rho[pt == 0] > 0).all()
    for out in (orc.dust_density(p, m, idx, pt, h), orc.num_dens(m, p, s["mu_array"], idx, d),
                orc.del_pressure(p, m, pt, idx, s["E_internal"], s["gamma_array"], d, return_abs_terms=True),
                orc.artificial_viscosity(idx, p, pt, h, m, rho, v, s["T"], s["gamma_array"], s["mu_array"], d,
                                         return_abs_terms=True),
                orc.net_impulse(p, m, h, v, pt, idx, s["f_un"], return_abs_terms=True) if loop_with_drag(K) else None):
        assert _all_finite(out)
    assert np.isfinite(orc.crossing_time(idx, v, h, pt))


# ---- the fused-step sweep ---------------------------------------------------------------------
# Cases that run under a fixed Courant step (ics.cfl_dt), as the Sedov cases do: under the reference's dt rule
# (dt >= dt_0 / 5, drv:226) the oracle itself sends them to inf / NaN within the three steps compared.
STEP_FIXED_DT = set()


def step_fixed_dt(case, s):
    import sph_code_amd.ics as ics
    return ics.cfl_dt(s, case[3]) if case in STEP_FIXED_DT else 0.0


@pytest.mark.parametrize("case", STEP_CASES, ids=case_id)
def test_step_sweep_case_is_not_vacuous(case):
    """Three oracle steps stay finite, the particles have moved and nothing has been flung beyond ten cloud sizes."""
    s0, d = case_state(*case[1:])
    fixed_dt = step_fixed_dt(case, s0)
    ref = dict(s0)
    for it in range(3):
        ref = oracle_step(case, ref, d, it == 0, fixed_dt)
    R0 = np.max(np.abs(s0["points"]))
    for key in ("points", "velocities", "sizes", "densities"):
        assert np.isfinite(ref[key]).all(), key
    assert np.max(np.abs(ref["points"])) < 10 * R0 and np.any(ref["points"] != s0["points"])
    assert np.any(ref["total_accel"] != 0)
