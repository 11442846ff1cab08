"""The transformed clouds of tests/frames.py are sound and the oracle holds on them alone (no GPU): the shifts and scalings
are exact, no case is vacuous (the oracle's outputs are finite on every row the GPU test compares - no frame drops a row,
and no frame needed another workload for that), exact distance ties stay below 1 % of the rows, and frames.grid_rule, the
NumPy restatement of DESIGN 5.1's grid sizing, does not depend on the frame."""
import numpy as np
import pytest

import frames
from oracle import sph_oracle as orc
from test_odd_shapes_cpu import _all_finite, hydro_modes, oracle_step

# (forms, frame, workload, N, K): the fused-step cases of tests/test_gpu_frames.py
# shift_12 of the polytrope (R0 = 2^63 m) lies beyond the reference's position clamp (1e11 AU = 1.5e22 m), which the step
# applies: the cases that carry that offset (shift_12, plane) take the first shape's N and K on the uniform cube (R0 = 2^57 m).
P, T, C = frames.SHAPES[0], frames.SHAPES[1], ("uniform_cube",) + frames.SHAPES[0][1:]
STEP_CASES = [("hydro_update", "shift_12") + C, ("hydro_update", "sheet") + P, ("hydro_update", "plane") + C,
              ("hydro_update", "needle") + P, ("hydro_update", "two_clumps") + P,
              ("loop", "shift_12") + T, ("loop", "two_clumps") + T, ("pairwise", "shift_12") + C]
# Cases that run under a fixed Courant step (ics.cfl_dt), as the Sedov cases do: under the reference's dt rule the oracle
# itself sends the exactly planar cube and the needle beyond ten cloud sizes within the three steps compared.
STEP_FIXED_DT = {STEP_CASES[2], STEP_CASES[3]}


def step_fixed_dt(case, s):
    """ics.cfl_dt with the cloud's own smallest kNN radius in place of the mean radius of a uniform fill of a ball, which
    a plane or a needle is not (their radii are orders of magnitude below it)."""
    import sph_code_amd.ics as ics
    if case not in STEP_FIXED_DT:
        return 0.0
    K = case[4]
    h = orc.neighbors(s["points"], np.inf, K, eps=0.0)[4]
    n = len(h)
    r = np.linalg.norm(s["points"] - s["points"].mean(axis=0), axis=1).max()
    return ics.cfl_dt(s, K) * float(h.min() / ((K / n) ** (1. / 3.) * r))


@pytest.mark.parametrize("case", [c for c in frames.CASES if c[0] in frames.SHIFTS + frames.SCALES], ids=frames.case_id)
def test_shift_and_scale_frames_are_exact(case):
    s, d, meta = frames.frame_case(*case)
    base = meta["base"]
    assert np.array_equal((s["points"] - meta["offset"]) / meta["scale"], base["points"])
    assert np.array_equal(s["velocities"] / meta["scale"], base["velocities"])
    assert d / meta["scale"] == meta["base_d"]
    k_ = np.round(base["points"] / meta["q"])
    assert np.array_equal(k_ * meta["q"], base["points"]) and np.abs(k_).max() <= 2 ** frames.Q_BITS
    # differences of a shifted cloud are the differences of the base cloud, bit for bit
    i, j = np.random.RandomState(1).randint(0, case[2], (2, 4000))
    assert np.array_equal(s["points"][i] - s["points"][j], (base["points"][i] - base["points"][j]) * meta["scale"])


@pytest.mark.parametrize("case", frames.CASES, ids=frames.case_id)
def test_frame_case_is_not_vacuous(case):
    """test_array_sweep_case_is_not_vacuous on the transformed cloud, unclamped (shift_20 and shift_27 lie beyond the
    reference's position clamp on purpose), plus the share of tied rows and distinct positions."""
    frame, workload, n, K = case
    s, d, meta = frames.frame_case(*case)
    p, v = s["points"], s["velocities"]
    if meta["kind"] == "clumps":
        assert len(np.unique(p, axis=0)) == n                     # the mirrored copy coincides with no particle of the first
    tied = frames.tied_rows(p, K)
    print("%s: %d of %d rows tied at the K-th distance" % (frames.case_id(case), tied.sum(), n))
    assert tied.sum() < 0.01 * n
    idx, _, _, nontriv, h = orc.neighbors(p, np.inf, K, eps=0.0)
    assert (nontriv == min(n, K)).all() and not (idx == n).any()
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
                orc.net_impulse(p, m, h, v, pt, idx, s["f_un"], return_abs_terms=True)):
        assert _all_finite(out)
    assert np.isfinite(orc.crossing_time(idx, v, h, pt))


@pytest.mark.parametrize("case", frames.CASES, ids=frames.case_id)
def test_grid_rule_does_not_depend_on_the_frame(case):
    frame, workload, n, K = case
    s, _, meta = frames.frame_case(*case)
    cell, nx, ny, nz = frames.grid_rule(s["points"], n, K)
    assert cell > 0 and 1 <= min(nx, ny, nz) and max(nx, ny, nz) <= 2047 and nx * ny * nz <= 32 * n + 1024
    if meta["kind"] in ("shift", "scale"):
        assert (cell / meta["scale"], nx, ny, nz) == frames.grid_rule(meta["base"]["points"], n, K)
    if frame == "clumps_shifted":
        assert (cell, nx, ny, nz) == frames.grid_rule(frames.frame_case("two_clumps", workload, n, K)[0]["points"], n, K)
    if frame in ("plane", "line"):                                 # an extent of exactly 0: one layer of cells
        assert nz == 1 and (frame == "plane" or ny == 1)


def test_grid_rule_clips_the_heavy_tailed_cloud():
    """The core + halo cloud of the GPU grid check: the 3 sigma clip is active there (the box is far smaller than the true
    bounding box) and the rule is the same 2^27 cloud sizes from the origin."""
    p, off = frames.heavy_tailed_cloud()
    n = len(p)
    g0, g1 = frames.grid_rule(p, n, 40), frames.grid_rule(p + off, n, 40)
    assert g0[1:] == g1[1:] and abs(g1[0] - g0[0]) <= 1e-12 * g0[0]
    assert g0[0] * max(g0[1:]) < 0.5 * np.ptp(p, axis=0).max()


@pytest.mark.parametrize("case", STEP_CASES, ids=frames.case_id)
def test_frame_step_case_is_not_vacuous(case):
    """test_step_sweep_case_is_not_vacuous on the transformed clouds: three oracle steps stay finite, the particles have
    moved and nothing has been flung beyond ten cloud sizes (measured from the cloud's own offset)."""
    s0, d, meta = frames.frame_case(*case[1:])
    fixed_dt = step_fixed_dt(case, s0)
    ref = dict(s0)
    for it in range(3):
        ref = oracle_step((case[0],) + case[2:], ref, d, it == 0, fixed_dt)
    # the cloud's extent about its own offset: R0 at most, except for the two clumps, which span 2^10 R0 by construction
    # (the GPU test gates positions by R0 itself)
    size = np.max(np.abs(s0["points"] - meta["offset"]))
    for key in ("points", "velocities", "sizes", "densities"):
        assert np.isfinite(ref[key]).all(), key
    assert np.max(np.abs(ref["points"] - meta["offset"])) < 10 * size and np.any(ref["points"] != s0["points"])
    assert np.any(ref["total_accel"] != 0)
