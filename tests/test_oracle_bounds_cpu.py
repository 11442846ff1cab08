"""The oracle's row chunking and its per-row sums of absolute terms (oracle/sph_oracle.py), which the full-size and
odd-shape GPU comparisons (tests/test_gpu_oracle_full_size.py, tests/test_gpu_odd_shapes.py) rest on; and the shapes
of the odd-shape sweep, checked here - oracle only, no GPU - not to be vacuous."""
import numpy as np
import pytest

from conftest import GOLDEN_CASES, hydro_args, load_golden
from oracle import sph_oracle as orc
from test_pairwise_cpu import viscosity_sums

CHUNKS = (512, 300)                # 300 divides none of the fixtures' N (256, 1024, 2048)


def _loop_calls(g, **kw):
    d = float(g["loop_d"])
    nb = g["nb_idx"].astype(np.int64)
    P, m, pt, h = g["points"], g["mass"], g["particle_type"], g["nb_h"]
    return dict(
        density=lambda: orc.density(P, m, pt, nb, d, **kw),
        dust_density=lambda: orc.dust_density(P, m, nb, pt, h, **kw),
        num_dens=lambda: orc.num_dens(m, P, g["mu_array"], nb, d, **kw),
        del_pressure=lambda **k2: orc.del_pressure(P, m, pt, nb, g["E_internal"], g["gamma_array"], d, **kw, **k2),
        artificial_viscosity=lambda **k2: orc.artificial_viscosity(nb, P, pt, h, m, g["loop_density"], g["velocities"],
                                                                   g["T"], g["gamma_array"], g["mu_array"], d, **kw, **k2),
        net_impulse=lambda **k2: orc.net_impulse(P, m, h, g["velocities"], pt, nb, g["f_un"], **kw, **k2),
        crossing_time=lambda: orc.crossing_time(nb, g["velocities"], h, pt, **kw))


def _same(a, b):
    a = a if isinstance(a, tuple) else (a,)
    b = b if isinstance(b, tuple) else (b,)
    return len(a) == len(b) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def test_chunked_loop_forms_are_bit_identical(golden):
    whole = {k_: f() for k_, f in _loop_calls(golden, chunk=None).items()}
    assert _same(whole["density"], _loop_calls(golden)["density"]())             # the default chunking too
    for chunk in CHUNKS:
        for k_, f in _loop_calls(golden, chunk=chunk).items():
            assert _same(whole[k_], f()), (k_, chunk)


@pytest.mark.parametrize("visc_mode", ["ref_axis0", "pairwise", "axis0_restated"])
def test_chunked_hydro_update_is_bit_identical(golden, visc_mode):
    args = hydro_args(golden)
    with np.errstate(all="ignore"):
        whole = orc.hydro_update(*args, chunk=1 << 30, visc_mode=visc_mode)
        for chunk in CHUNKS:
            assert _same(whole, orc.hydro_update(*args, chunk=chunk, visc_mode=visc_mode)), chunk
        rows, inter = orc.hydro_update(*args, chunk=300, visc_mode=visc_mode, return_intermediates="rows")
        full, inter_full = orc.hydro_update(*args, chunk=512, visc_mode=visc_mode, return_intermediates=True)
    assert _same(whole, rows) and _same(whole, full)                              # asking for the bounds changes no sum
    for k_ in ("G_abs_terms", "visc_abs_terms", "visc_heat_abs_terms"):
        assert np.array_equal(inter[k_], inter_full[k_], equal_nan=True), k_
    assert not any(np.ndim(v) == 2 and v.shape[1] == args[0].shape[1] and v.shape[1] != 3 for v in inter.values())


@pytest.mark.parametrize("case", GOLDEN_CASES)
@pytest.mark.parametrize("clip_grad", [False, True])
def test_chunked_pairwise_restatement_is_bit_identical(case, clip_grad):
    args = hydro_args(load_golden(case))
    out_a, pi_a = viscosity_sums(args, clip_grad=clip_grad, chunk=512)
    out_b, pi_b = viscosity_sums(args, clip_grad=clip_grad, chunk=300)
    assert _same(out_a, out_b) and np.array_equal(pi_a, pi_b, equal_nan=True)
    out_c, rows = viscosity_sums(args, clip_grad=clip_grad, chunk=300, per_pair=False)
    assert _same(out_a, out_c) and set(rows) >= {"visc_abs_terms", "visc_heat_abs_terms"}


def _dominates(abs_sum, signed, what):
    """sum_k|t_k| >= |sum_k t_k| row by row (the two are summed in the same order, up to the nesting of the heat's
    dot product: a few ulp of slack), with the same non-finite pattern."""
    fin = np.isfinite(signed)
    assert (np.isfinite(abs_sum) == fin).all(), what
    assert (abs_sum[fin] >= 0).all() and (abs_sum[fin] * (1 + 1e-14) >= np.abs(signed[fin])).all(), what
    assert (abs_sum[fin] > 0).any(), what + ": bound is zero everywhere"


@pytest.mark.parametrize("visc_mode", ["ref_axis0", "pairwise"])
def test_hydro_update_abs_terms_bound_their_sums(golden, visc_mode):
    with np.errstate(all="ignore"):
        out, inter = orc.hydro_update(*hydro_args(golden), return_intermediates="rows", visc_mode=visc_mode)
    _dominates(inter["G_abs_terms"], inter["pressure_grad_symmetrized"].T, "G")
    _dominates(inter["visc_abs_terms"], out[1], "visc_accel")
    _dominates(inter["visc_heat_abs_terms"], out[2], "visc_heat")


def test_loop_form_abs_terms_bound_their_sums_and_leave_them_untouched(golden):
    calls = _loop_calls(golden)
    dp, dp_abs = calls["del_pressure"](return_abs_terms=True)
    assert np.array_equal(dp, calls["del_pressure"]())
    _dominates(dp_abs, dp, "del_pressure")
    acc, heat, acc_abs, heat_abs = calls["artificial_viscosity"](return_abs_terms=True)
    assert _same((acc, heat), calls["artificial_viscosity"]())
    _dominates(acc_abs, acc, "av accel")
    _dominates(heat_abs, heat, "av heat")
    onto, react, onto_abs, react_abs = calls["net_impulse"](return_abs_terms=True)
    assert _same((onto, react), calls["net_impulse"]())
    if (golden["particle_type"] == 2).any():
        _dominates(onto_abs, onto, "drag onto")
        _dominates(react_abs, react, "drag reaction")
    else:
        assert not onto_abs.any() and not react_abs.any()
    # the signed sums are still the fixture's
    assert np.max(np.abs(dp - golden["loop_del_pressure"])) <= 1e-10 * np.max(np.abs(golden["loop_del_pressure"]))


def test_loop_forms_missing_neighbours_contribute_zero(golden):
    """idx == N (nsc:545-548) adds nothing: five-entry lists (NumPy sums fewer than 8 terms in sequence) with and
    without a trailing missing column give the same bits."""
    g = dict(golden)
    n = len(g["points"])
    short = g["nb_idx"].astype(np.int64)[:, :5]
    g["nb_idx"] = short
    base = {k_: f() for k_, f in _loop_calls(g).items()}
    g["nb_idx"] = np.concatenate([short, np.full((n, 1), n, np.int64)], axis=1)
    for k_, f in _loop_calls(g).items():
        assert _same(base[k_], f()), k_
