"""Row-by-row comparison of the array API's sums with the CPU oracle (test helper, no test of its own).

Tolerances are SURVEY 8c's, as tests/test_gpu_parity.py states them:
  sums of <= K non-negative terms      rtol 1e-13 (1e-12 for the loop-form densities), atol 0, every row
  signed sums                          per row and component |x - ref| <= 1e-12 sum_k|term_k| + 4e-16 |ref|
                                       (the expression of test_hydro_update_termwise_bound); where sum_k|term_k| is
                                       exactly 0 the two are equal; and, beside it, the max-norm gate
                                       |x - ref| <= 1e-10 max|ref| the small tests state
The oracle side runs `chunk` rows at a time, so its peak is a few (chunk, K, 3) arrays at any N.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import sph_oracle as orc

RTOL_POS = 1e-13
RTOL_LOOP_POS = 1e-12
RTOL_SIGNED = 1e-10
TERM_TOL = 1e-12
REF_TOL = 4e-16


def pos_close(x, ref, what, rtol=RTOL_POS):
    """Non-negative sums: every row, rtol, atol 0; the reference finite everywhere.  -> rows compared."""
    x, ref = np.asarray(x), np.asarray(ref)
    assert x.shape == ref.shape, what
    assert np.isfinite(ref).all(), "%s: oracle not finite on %d rows" % (what, (~np.isfinite(ref)).sum())
    err = np.abs(x - ref)
    bad = ~(err <= rtol * np.abs(ref))
    with np.errstate(all="ignore"):
        worst = np.max(np.where(ref != 0, err / np.abs(ref), np.where(err == 0, 0., np.inf))) if ref.size else 0.0
    rows = ref.shape[-1]                                # (N,) or, for the species sums, (S, N)
    print("%-34s rows compared %8d  worst rel err %.3g (gate %.0e)" % (what, rows, worst, rtol))
    assert not bad.any(), "%s: %d elements off, worst rel %.3g" % (what, bad.sum(), worst)
    return rows


def rows_close(x, ref, scale, what, nonfinite_rows_allowed=False):
    """Signed sums, per row and component, against scale = sum_k|term_k| (same shape as ref).
    nonfinite_rows_allowed=False: the reference must be finite everywhere (nothing is left out).
    True: the non-finite pattern of x and ref must be identical and every finite element is compared.
    Prints the rows compared and the worst |x - ref| / (1e-12 sum|term|).  -> rows compared."""
    x, ref, scale = np.asarray(x), np.asarray(ref), np.asarray(scale)
    assert x.shape == ref.shape == scale.shape, what
    fin = np.isfinite(ref)
    if not nonfinite_rows_allowed:
        assert fin.all(), "%s: oracle not finite on %d elements" % (what, (~fin).sum())
    assert (np.isfinite(x) == fin).all(), "%s: non-finite pattern differs on %d elements" % (
        what, (np.isfinite(x) != fin).sum())
    assert np.isfinite(scale[fin]).all(), "%s: a finite sum with a non-finite sum of |terms|" % what
    rows = int(fin.all(axis=1).sum()) if ref.ndim == 2 else int(fin.sum())
    if not fin.any():
        print("%-34s rows compared %8d" % (what, 0))
        return 0
    xf, rf, sf = x[fin], ref[fin], scale[fin]
    err = np.abs(xf - rf)
    zero = sf == 0
    assert (xf[zero] == rf[zero]).all(), "%s: %d elements differ where every term is zero" % (
        what, (xf[zero] != rf[zero]).sum())
    ratio = np.zeros_like(err)
    ratio[~zero] = err[~zero] / (TERM_TOL * sf[~zero])
    worst = float(ratio.max())
    print("%-34s rows compared %8d  worst |x-ref|/(1e-12 sum|term|) %.3g" % (what, rows, worst))
    bad = ~(err <= TERM_TOL * sf + REF_TOL * np.abs(rf))
    assert not bad.any(), "%s: %d elements beyond the per-row bound, worst ratio %.3g" % (what, bad.sum(), worst)
    assert err.max() <= RTOL_SIGNED * np.abs(rf).max(), what + " (max-norm)"
    return rows


def hydro_reference(args, clip_grad=False, visc_mode="ref_axis0", chunk=32768):
    """oracle.hydro_update on `args` -> (the seven outputs, {output index: sum_k|term_k| of that signed sum})."""
    with np.errstate(all="ignore"):
        ref, inter = orc.hydro_update(*args, return_intermediates="rows", clip_grad=clip_grad, visc_mode=visc_mode,
                                      chunk=chunk)
        scales = {0: inter["G_abs_terms"] / ref[3][:, None],            # hydro_accel = G / rho
                  1: inter["visc_abs_terms"], 2: inter["visc_heat_abs_terms"]}
    return ref, scales


HYDRO_NAMES = ("hydro_accel", "visc_accel", "visc_heat", "density", "num_density", "f_un_neighbor", "dust_density")


def compare_hydro(out, ref, scales, label, which=(0, 1, 2, 3, 4, 5, 6), visc_nonfinite_ok=False):
    """All rows of the outputs `which` of hydro_update.  -> {name: rows compared}."""
    n = len(ref[3])
    seen = {}
    for i in which:
        what = "%s %s" % (label, HYDRO_NAMES[i])
        if i in (0, 1, 2):
            seen[HYDRO_NAMES[i]] = rows_close(out[i], ref[i], scales[i], what,
                                              nonfinite_rows_allowed=visc_nonfinite_ok and i in (1, 2))
        else:
            seen[HYDRO_NAMES[i]] = pos_close(out[i], ref[i], what)
        if not (visc_nonfinite_ok and i in (1, 2)):
            assert seen[HYDRO_NAMES[i]] == n, (what, seen[HYDRO_NAMES[i]], n)
    return seen


def loop_reference(p, v, m, pt, h, idx, d, E, T, gam, mu, rho_for_av, f_un=None, chunk=32768, workers=6):
    """The oracle's loop forms on one state -> dict name -> (reference, sum_k|term_k| or None).  rho_for_av: the density
    array handed to artificial_viscosity (the driver passes the one nsc.density returned, drv:451,458).
    The forms are independent of each other and NumPy releases the GIL: they run side by side."""
    jobs = {
        "density": lambda: (orc.density(p, m, pt, idx, d, chunk=chunk), None),
        "dust_density": lambda: (orc.dust_density(p, m, idx, pt, h, chunk=chunk), None),
        "num_dens": lambda: (orc.num_dens(m, p, mu, idx, d, chunk=chunk), None),
        "del_pressure": lambda: orc.del_pressure(p, m, pt, idx, E, gam, d, chunk=chunk, return_abs_terms=True),
        "artificial_viscosity": lambda: orc.artificial_viscosity(idx, p, pt, h, m, rho_for_av, v, T, gam, mu, d,
                                                                 chunk=chunk, return_abs_terms=True),
        "crossing_time": lambda: (orc.crossing_time(idx, v, h, pt, chunk=chunk), None),
    }
    if f_un is not None:
        jobs["net_impulse"] = lambda: orc.net_impulse(p, m, h, v, pt, idx, f_un, chunk=chunk, return_abs_terms=True)
    with ThreadPoolExecutor(max_workers=workers) as ex:
        futs = {k_: ex.submit(fn) for k_, fn in jobs.items()}
        return {k_: f.result() for k_, f in futs.items()}


def compare_loop(nsc, ref, p, v, m, pt, h, idx, d, E, T, gam, mu, rho_for_av, label, f_un=None):
    """The array API's loop forms on the same arguments against `ref` (loop_reference), every row."""
    n = len(p)
    nsc.d = d
    assert pos_close(nsc.density(p, m, pt, idx), ref["density"][0], label + " density", RTOL_LOOP_POS) == n
    assert pos_close(nsc.dust_density(p, m, idx, pt, h), ref["dust_density"][0], label + " dust_density",
                     RTOL_LOOP_POS) == n
    assert pos_close(nsc.num_dens(m, p, mu, idx), ref["num_dens"][0], label + " num_dens", RTOL_LOOP_POS) == n
    dp, dp_abs = ref["del_pressure"]
    assert rows_close(nsc.del_pressure(p, m, pt, idx, E, gam), dp, dp_abs, label + " del_pressure") == n
    acc, heat, acc_abs, heat_abs = ref["artificial_viscosity"]
    gacc, gheat = nsc.artificial_viscosity(idx, p, pt, h, m, rho_for_av, v, T, gam, mu)
    assert rows_close(gacc, acc, acc_abs, label + " av accel") == n
    assert rows_close(gheat, heat, heat_abs, label + " av heat") == n
    ct, ct_ref = nsc.crossing_time(idx, v, h, pt), ref["crossing_time"][0]
    assert abs(ct - ct_ref) <= 1e-14 * abs(ct_ref), (label, ct, ct_ref)
    if f_un is not None:
        onto, react, onto_abs, react_abs = ref["net_impulse"]
        gonto, greact = nsc.net_impulse(p, m, h, v, pt, idx, f_un)
        assert rows_close(gonto, onto, onto_abs, label + " drag onto") == n
        assert rows_close(greact, react, react_abs, label + " drag reaction") == n
        return gonto, greact
    return None
