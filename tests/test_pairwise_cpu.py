"""The pairwise artificial viscosity (hydro_update visc_mode="pairwise", include/sphx.h sphx_hydro_update): a NumPy
restatement of its sums built from the oracle's public pieces, anchored on the golden fixtures, and the Python layer's
argument checks.  No GPU needed.

Pairwise:   B_ik = 1/2 pi_ik [m_j g_j gb + m_i g_i ga]            (pi_ik = the nsc:649 term, inside the sum)
ref_axis0:  B_ik = 1/2 [m_j g_j Pi_j gb + m_i g_i Pi_i ga]        (Pi_i = sum_k pi_ik, the oracle's mode)
visc_accel_i = -sum_k B_ik,  visc_heat_i = (m_i/2) sum_k B_ik . dv
"""
import numpy as np
import pytest

from conftest import GOLDEN_CASES, hydro_args, load_golden
from oracle import sph_oracle as orc


def pair_pi(w, rho_ab, c_ab):
    """nsc:649 per pair, alpha = 1."""
    with np.errstate(all="ignore"):
        return -1. / 2. * (c_ab * 2 - 3 * w) * w / rho_ab


def viscosity_sums(args, clip_grad=False, mode="pairwise", chunk=32768, per_pair=True):
    """-> (oracle outputs with visc_accel, visc_heat replaced by the `mode` sums, per-pair pi (N,K)).
    mode "axis0": the same code with pi_ik replaced by Pi_j (neighbour term) and Pi_i (own term).
    The sums are the oracle's (hydro_update visc_mode="pairwise" / "axis0_restated"), formed `chunk` rows at a time;
    per_pair=False returns, in place of pi, the per-row bounds alone (visc_abs_terms = sum_k |B_ik|,
    visc_heat_abs_terms = sum_k |B_ik . dv| m_i / 2, G_abs_terms) - nothing of size (N, K) is kept."""
    visc_mode = {"pairwise": "pairwise", "axis0": "axis0_restated"}[mode]
    with np.errstate(all="ignore"):
        out, inter = orc.hydro_update(*args, return_intermediates=True if per_pair else "rows", clip_grad=clip_grad,
                                      visc_mode=visc_mode, chunk=chunk)
    return out, (inter["pi"] if per_pair else inter)


def signed_close(x, ref, what, tol=1e-10):
    fin = np.isfinite(ref)
    assert (np.isfinite(x) == fin).all(), what
    assert np.max(np.abs(x - ref)[fin]) <= tol * np.max(np.abs(ref[fin])), what


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_restatement_reproduces_the_fixture_in_axis0_form(case):
    """The restatement's plumbing: with Pi_j / Pi_i in place of pi_ik it is the reference's captured sums."""
    g = load_golden(case)
    out, _ = viscosity_sums(hydro_args(g), mode="axis0")
    signed_close(out[1], g["hu_visc_accel"], "visc_accel " + case)
    signed_close(out[2], g["hu_visc_heat"], "visc_heat " + case)


def test_pair_pi_matches_the_reference_capture():
    g = load_golden("small_n256_k16")
    _, pi = viscosity_sums(hydro_args(g))
    # the capture is (K, N): the transpose of the oracle's layout
    ref = pair_pi(g["cap_w_ab"].T, g["cap_rho_avg_ab"].T, g["cap_c_sound_ab"].T)
    valid = g["nb_idx"] < len(g["nb_idx"])
    np.testing.assert_allclose(pi[valid], ref[valid], rtol=1e-13, atol=0)


@pytest.mark.parametrize("case", GOLDEN_CASES)
@pytest.mark.parametrize("clip_grad", [False, True])
def test_pairwise_heat_is_never_negative(case, clip_grad):
    """The property the axis-0 mode lacks: visc_heat >= 0 for every particle."""
    g = load_golden(case)
    out, _ = viscosity_sums(hydro_args(g), clip_grad=clip_grad)
    assert np.isfinite(out[2]).all() and (out[2] >= 0).all(), case


def test_visc_mode_argument_errors():
    import sph_code_amd.compat as nsc
    from sph_code_amd.sim import Simulation
    from sph_code_amd import multigpu as mg
    g = load_golden("small_n256_k16")
    for bad in ("Pairwise", "loop", 1, None):
        with pytest.raises(ValueError):
            nsc.hydro_update(*hydro_args(g), visc_mode=bad)
    state = dict(points=g["points"], velocities=g["velocities"], mass=g["mass"], particle_type=g["particle_type"],
                 T=g["T"], mu_array=g["mu_array"], gamma_array=g["gamma_array"], E_internal=g["E_internal"])
    with pytest.raises(ValueError):
        Simulation(state, n_neigh=16, forms="loop", d=1e18, visc_mode="pairwise")
    with pytest.raises(ValueError):
        Simulation(state, n_neigh=16, visc_mode="bogus")
    with pytest.raises(ValueError):
        mg.DistributedSim(state, None, None, None, forms="loop", d=1e18, visc_mode="pairwise")
    with pytest.raises(ValueError):
        mg.DistributedSim(state, None, None, object(), visc_mode="pairwise")      # a backend without visc_pairwise
