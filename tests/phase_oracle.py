"""NumPy restatement of the dust phase of the reference's time loop (code_running.py:399-435) - the yardstick of the
phase tests.  Written from the formulas (include/sphx.h, sphx_dust_bookkeeping and sphx_state_dust_phase), not from the
driver's text.  The two ordered stages are chem_oracle's and dust_oracle's; the density is the oracle's loop form.

    normalise     every row of f_un divided by its sum                                              drv:399, 424
    bookkeeping   delta_n = nan_to_num(reup - destr) in longdouble; mass_change = nan_to_num(sum_t mass / mu delta_n mu_specie);
                  f_un += delta_n, NaN -> 1e-15, rows renormalised; mass += mass_change, a negative mass -> crit_mass / 200;
                  mu = sum f mu_specie / sum f, gamma = sum f gamma / sum f                         drv:412-433
    chain         normalise, density, chemisputtering, sputtering on its outputs, bookkeeping - each stage on the previous
                  stages' outputs, or, `given` a stage's outputs from elsewhere (the reference's own), on those

Precision: the driver holds mass and f_un in longdouble (drv:153-155) and casts delta_n to it (drv:416); so does
`bookkeeping`, whatever it is handed, and returns float64.  The library works in double throughout.

Bounds, derived, not tuned, first order in TAU = 1e-12 sum|terms| (the project's bound for a sum that may be evaluated in
another order or precision):
    v_t = f_t + delta_t                    dv_t = TAU (|f_t| + |delta_t|)
    tot = sum_t v_t                        dtot = sum_t dv_t + TAU sum_t |v_t|
    f_out_t = v_t / tot                    df_t = dv_t / |tot| + |v_t| dtot / tot^2 + TAU |f_out_t|
    mass_change = sum_t r delta_t mus_t    dchg = TAU sum_t |r delta_t mus_t|
    mass_out = mass + mass_change          dm = dchg + TAU (|mass| + |mass_change|)
    mu_out = A / B, A = sum f_out mus, B = sum f_out:  dA = sum df mus + TAU sum |f_out mus|, dB = sum df + TAU sum |f_out|,
                                           dmu = dA / |B| + |A| dB / B^2 + TAU |mu_out|; gamma likewise
A row whose NaN entries were filled carries the same bounds (1e-15 is exact).  Decisions: a mass is reset when
mass_out < 0; `reset_margin` is min |mass_out| / dm over all particles before the reset - 1e6 or more means no reset can
fall the other way in the library; the NaN fills depend on NaN-ness alone, which no rounding changes.
"""
import numpy as np

import chem_oracle
import dust_oracle
from oracle import sph_oracle as orc

LD = np.longdouble
TAU = 1e-12
GAMMA = np.array([7. / 5, 5. / 3, 5. / 3, 5. / 3, 5. / 3, 5. / 3, 5. / 3, 15.6354113, 4.913, 1.0125, 2.364, 3.02, 10., 10., 10.])
BOOK_OUTPUTS = ("mass", "f_un", "mu_array", "gamma_array")
TOTALS = ("mass_before", "mass_after_chem", "mass_after", "mass_reduction", "mass_increase", "mass_change")


def gamma_table(S):
    """The driver's gamma (drv:51) cut to S, or padded with 5/3."""
    return GAMMA[:S].copy() if S <= len(GAMMA) else np.concatenate([GAMMA, np.full(S - len(GAMMA), 5. / 3)])


def normalise(f_un):
    f = np.asarray(f_un)
    return f / np.sum(f, axis=1)[:, None]


def numpy_row_sum(a):
    """np.sum(a, axis=1) of a C-contiguous (n, s) float64 array with s < 128, written out: NumPy adds such a row with eight
    running sums over the whole blocks of eight, combines them pairwise and adds the rest one by one; below eight entries
    it adds them in order.  The library's drag refresh adds a row in this order so that its mean_grain_mass and mean_cross
    are what Simulation forms from the same f_un with np.sum; tests/test_phase_cpu.py holds this restatement to the
    installed NumPy, so a NumPy that adds otherwise is found there and not on the GPU."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    s = a.shape[1]
    if s < 8:
        res = np.zeros(a.shape[0])
        for t in range(s):
            res = res + a[:, t]
        return res
    r = [a[:, j].copy() for j in range(8)]
    t = 8
    while t < s - s % 8:
        for j in range(8):
            r[j] = r[j] + a[:, t + j]
        t += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for u in range(t, s):
        res = res + a[:, u]
    return res


def _fin(a):
    return np.where(np.isfinite(a), a, 0.0)


def bookkeeping(mass, mu_array, f_un, frac_destruction, frac_reuptake, mu_specie, gamma, crit_mass, mass_before=None):
    """-> dict: mass, f_un, mu_array, gamma_array (float64), "<name>_bound", totals and totals_bound (dicts over TOTALS),
    reset (indices of the masses reset), filled (indices (i, t) of the NaN entries filled), reset_margin."""
    m = np.asarray(mass).astype(LD)
    f = np.asarray(f_un).astype(LD)
    mu = np.asarray(mu_array, dtype=np.float64)
    fd, fr = np.asarray(frac_destruction, dtype=np.float64), np.asarray(frac_reuptake, dtype=np.float64)
    mus, gam = np.asarray(mu_specie, dtype=np.float64), np.asarray(gamma, dtype=np.float64)
    with np.errstate(all="ignore"):
        r = m / mu
        delta = np.nan_to_num(fr - fd).astype(LD)
        terms = r[:, None] * delta * mus
        chg = np.nan_to_num(np.sum(terms, axis=1))
        chg_b = TAU * _fin(np.sum(np.abs(terms), axis=1)).astype(np.float64)
        red_i = np.sum(r[:, None] * fd * mus, axis=1)
        inc_i = np.sum(r[:, None] * fr * mus, axis=1)
        v = f + delta
        filled = np.argwhere(np.isnan(v))
        v_b = TAU * _fin(np.abs(f) + np.abs(delta)).astype(np.float64)
        v = np.where(np.isnan(v), LD(1e-15), v)
        tot = np.sum(v, axis=1)
        tot_b = np.sum(v_b, axis=1) + TAU * np.sum(np.abs(v), axis=1).astype(np.float64)
        f_out = v / tot[:, None]
        atot = np.abs(tot).astype(np.float64)[:, None]
        f_b = v_b / atot + np.abs(v).astype(np.float64) * tot_b[:, None] / atot ** 2 + TAU * np.abs(f_out).astype(np.float64)
        m_out = m + chg
        m_b = chg_b + TAU * (np.abs(m) + np.abs(chg)).astype(np.float64)
        reset = np.nonzero(m_out < 0)[0]
        live = m_b > 0
        reset_margin = float(np.min(np.abs(m_out[live]).astype(np.float64) / m_b[live])) if live.any() else np.inf
        m_fin = np.where(m_out < 0, LD(crit_mass / 200.), m_out)
        out = dict(mass=m_fin.astype(np.float64), mass_bound=np.where(m_out < 0, 0.0, m_b), f_un=f_out.astype(np.float64),
                   f_un_bound=f_b)
        B = np.sum(f_out, axis=1)
        B_b = np.sum(f_b, axis=1) + TAU * np.sum(np.abs(f_out), axis=1).astype(np.float64)
        aB = np.abs(B).astype(np.float64)
        for name, tab in (("mu_array", mus), ("gamma_array", gam)):
            A = np.sum(f_out * tab, axis=1)
            A_b = np.sum(f_b * np.abs(tab), axis=1) + TAU * np.sum(np.abs(f_out * tab), axis=1).astype(np.float64)
            q = A / B
            out[name] = q.astype(np.float64)
            out[name + "_bound"] = A_b / aB + np.abs(A).astype(np.float64) * B_b / aB ** 2 + TAU * np.abs(q).astype(np.float64)
        mb = None if mass_before is None else np.asarray(mass_before).astype(LD)
        sums = dict(mass_before=mb, mass_after_chem=m, mass_after=m_fin, mass_reduction=-red_i, mass_increase=inc_i,
                    mass_change=chg)
        totals, totals_b = {}, {}
        for name, a in sums.items():
            totals[name] = float(np.sum(a)) if a is not None else float("nan")
            totals_b[name] = TAU * float(np.sum(np.abs(_fin(a)))) if a is not None else 0.0
        # the per-particle terms of the last three are sums over species themselves
        for name, fr_ in (("mass_reduction", fd), ("mass_increase", fr), ("mass_change", delta)):
            totals_b[name] += TAU * float(np.sum(np.abs(_fin(r[:, None] * fr_ * mus))))
    out.update(totals=totals, totals_bound=totals_b, reset=reset, filled=filled, reset_margin=reset_margin)
    return out


def chain(points, velocities, neighbor, mass, f_un, mu_array, sizes, T, particle_type, d, dt, crit_mass, guard="fraction",
          mu_specie=None, gamma=None, critical_density=dust_oracle.CRITICAL_DENSITY, amu=chem_oracle.AMU, given=None, model=True,
          **chem_kw):
    """The block, stage by stage -> dict: f_un_normalised, density, chem (chem_oracle.sputter's dict), dust
    (dust_oracle.destruction's dict), book (bookkeeping's dict).  given: {"density": ..., "mass_chem": ..., "f_un_chem": ...,
    "frac_destruction": ..., "frac_reuptake": ...} - a later stage then runs on these instead of this chain's own."""
    given = given or {}
    S = np.shape(f_un)[1]
    mus = chem_oracle.tables(S)[0] if mu_specie is None else np.asarray(mu_specie, dtype=np.float64)
    gam = gamma_table(S) if gamma is None else np.asarray(gamma, dtype=np.float64)
    out = dict(f_un_normalised=normalise(np.asarray(f_un, dtype=np.float64)))
    out["density"] = orc.density(points, mass, particle_type, neighbor, d)
    out["chem"] = chem_oracle.sputter(points, neighbor, mass, out["f_un_normalised"], mu_array, sizes, T, particle_type, d=d, dt=dt,
                                      model=model, mu_specie=mus, amu=amu, **chem_kw)
    m1 = given.get("mass_chem", out["chem"]["mass_new"])
    f1 = given.get("f_un_chem", out["chem"]["f_un_new"])
    out["dust"] = dust_oracle.destruction(points, velocities, neighbor, m1, f1, mu_array, sizes, given.get("density", out["density"]),
                                          particle_type, crit_mass=crit_mass, critical_density=critical_density, guard=guard,
                                          amu=amu)
    out["book"] = bookkeeping(m1, mu_array, f1, given.get("frac_destruction", out["dust"]["frac_destruction"]),
                              given.get("frac_reuptake", out["dust"]["frac_reuptake"]), mus, gam, crit_mass, mass_before=mass)
    return out


def conditions(ch, mass):
    """What every input set used for an oracle comparison must meet (conditions, not thresholds: change the seed if one
    fails) -> dict of the figures; raises AssertionError naming the first that fails."""
    c, dcounts = ch["chem"]["counts"], ch["dust"]["counts"]
    moved = int(np.count_nonzero(np.abs(ch["book"]["mass"] - np.asarray(mass, dtype=np.float64)) > 1e-6 * np.abs(mass)))
    fig = dict(rows=c["rows"], rounds=c["rounds"], accepted=dcounts["accepted"], chem_slack=min(ch["chem"]["slack"].values()),
               dust_slack=min(ch["dust"]["slack"].values()), moved=moved)
    assert fig["rows"] > 0 and fig["rounds"] is not None and fig["rounds"] >= 3 and fig["accepted"] > 0, fig
    assert fig["chem_slack"] >= 1e6 and fig["dust_slack"] >= 1e6, fig
    assert fig["moved"] >= 1000, fig
    return fig
