"""NumPy restatement of the census, the ordered selections, the stellar clock and the schedule (include/sphx.h, sphx_census
and its neighbours): the per-row terms with the driver's expressions (drv:616-617, 636, 656-658, 465-468), summed over the
particle index in the order of the library's ordered totals, which tests/sn_oracle.ordered_total states one value at a
time and ordered_totals here states for many quantities at once (test_census_cpu.py holds the two against each other).

Nothing here is tuned to the library's output: every line follows the reference's statement or the header's rule."""
import numpy as np

TOT_CHUNK = 256
TOT_LANES = 256
FIXED = 13
SOLAR_MASS = 1.989e30            # nsc:30
YEAR = 60. * 60. * 24. * 365.    # nsc:31
MU_SPECIE = np.array([2.0158, 4.0026, 1.0079, 1.0074, 4.0021, 4.0016, 0.0005, 140.69, 60.08, 12.0107,
                      28.0855, 55.834, 100.39, 131.93, 40.096])          # nsc:41


def ordered_totals(terms):
    """Row-wise sums of terms (nq, n) in sphx_ordered_totals' order: chunks of 256 consecutive entries left to right (a
    short last chunk padded with +0.0, which leaves a sum that started from +0.0 as it is); lane l of 256 adds the chunks
    l, l + 256, ... in order; the lanes by a binary tree."""
    v = np.atleast_2d(np.asarray(terms, dtype=np.float64))
    nq, n = v.shape
    nchunk = (n + TOT_CHUNK - 1) // TOT_CHUNK
    pad = np.zeros((nq, nchunk * TOT_CHUNK))
    pad[:, :n] = v
    pad = pad.reshape(nq, nchunk, TOT_CHUNK)
    with np.errstate(all="ignore"):
        part = np.zeros((nq, nchunk))
        for j in range(TOT_CHUNK):
            part = part + pad[:, :, j]
        rounds = (nchunk + TOT_LANES - 1) // TOT_LANES
        pp = np.zeros((nq, rounds * TOT_LANES))
        pp[:, :nchunk] = part
        pp = pp.reshape(nq, rounds, TOT_LANES)
        lanes = np.zeros((nq, TOT_LANES))
        for r in range(rounds):
            lanes = lanes + pp[:, r, :]
        h = TOT_LANES // 2
        while h > 0:
            lanes = lanes[:, :h] + lanes[:, h:2 * h]
            h //= 2
    return lanes[:, 0].copy()


def terms(mass, particle_type, f_un=None, mu_specie=None, velocities=None, total_accel=None, E_internal=None):
    """The per-row terms (13 + 3 S, n), a row outside a quantity's mask +0.0 by selection (np.where picks, it does not
    multiply)."""
    m = np.asarray(mass, dtype=np.float64)
    pt = np.asarray(particle_type, dtype=np.float64)
    n = m.shape[0]
    S = 0 if f_un is None else np.shape(f_un)[1]
    v = np.zeros((n, 3)) if velocities is None else np.asarray(velocities, dtype=np.float64)
    a = np.zeros((n, 3)) if total_accel is None else np.asarray(total_accel, dtype=np.float64)
    E = np.zeros(n) if E_internal is None else np.asarray(E_internal, dtype=np.float64)
    out = np.zeros((FIXED + 3 * S, n))
    with np.errstate(all="ignore"):
        out[0] = np.where(pt == 0, m, 0.0)
        out[1] = np.where(pt == 1, m, 0.0)
        out[2] = np.where(pt == 2, m, 0.0)
        out[3] = np.where(pt != 2, m, 0.0)
        out[4] = m
        for c in range(3):
            out[5 + c] = m * a[:, c]
            out[8 + c] = m * v[:, c]
        out[11] = m * ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        out[12] = E
        if S:
            fm = np.asarray(f_un, dtype=np.float64) * np.asarray(mu_specie, dtype=np.float64)
            for ty in range(3):
                mask = pt == ty
                # drv:656-658 on the rows of the type: ((f mu).T / np.sum(f mu, axis=1)) * mass
                sel = np.ascontiguousarray(fm[mask])
                t = ((sel.T / np.sum(sel, axis=1)) * m[mask])
                out[FIXED + ty * S:FIXED + (ty + 1) * S][:, mask] = t
    return out


def census(mass, particle_type, f_un=None, mu_specie=None, velocities=None, total_accel=None, E_internal=None):
    """-> dict with the keys of compat.census that the tests compare."""
    m = np.asarray(mass, dtype=np.float64)
    pt = np.asarray(particle_type, dtype=np.float64)
    S = 0 if f_un is None else np.shape(f_un)[1]
    tot = ordered_totals(terms(m, pt, f_un, mu_specie, velocities, total_accel, E_internal))
    n_star, n_nondust = int(np.count_nonzero(pt == 1)), int(np.count_nonzero(pt != 2))
    out = dict(gas_mass=tot[0], star_mass=tot[1], dust_mass=tot[2], nondust_mass=tot[3], total_mass=tot[4],
               n_gas=int(np.count_nonzero(pt == 0)), n_star=n_star, n_dust=int(np.count_nonzero(pt == 2)), n_nondust=n_nondust,
               max_star_mass=float(np.max(m[pt == 1])) if n_star else None, mass_accel=tot[5:8], momentum=tot[8:11],
               kinetic=0.5 * tot[11], internal=tot[12])
    with np.errstate(all="ignore"):
        out["star_massfrac"] = float(np.float64(tot[1]) / np.float64(tot[3]))            # drv:616 from the two sums
        out["star_numfrac"] = float(np.float64(n_star) / np.float64(n_nondust))          # drv:617
        out["net_accel"] = tot[5:8] / tot[4]
    for q, nm in enumerate(("gas_mass_by_species", "star_mass_by_species", "dust_mass_by_species")):
        out[nm] = tot[FIXED + q * S:FIXED + (q + 1) * S] if S else None
    return out


def sum_bound(term_row, n_t):
    """|got - ref| <= 2 n_t 2^-53 sum|term| between two summation orders of the same n_t terms: each side's standard
    bound (n_t - 1) u sum|term|, u = 2^-53, added up."""
    return 2.0 * n_t * 2.0 ** -53 * float(np.sum(np.abs(term_row)))


def advance(star_ages, particle_type, dt):
    """drv:604."""
    a = np.array(star_ages, dtype=np.float64)
    pt = np.asarray(particle_type, dtype=np.float64)
    a[(pt == 1) & (a > -2)] += dt
    return a


def lifetime(base_imf):
    """nsc:174-200 with lifetime = 1: stellar lifetimes in units of 1e10 years, floored at 3.6e-4."""
    b = np.asarray(base_imf, dtype=np.float64)
    expo = np.zeros(len(b)); coeff = np.zeros(len(b))
    expo[b < 0.7] = 2.62; expo[b >= 0.7] = 3.92
    coeff[b < 0.7] = 0.35; coeff[b >= 0.7] = 1.02
    with np.errstate(all="ignore"):
        life = coeff ** (-1) * b ** (1 - expo)
    life[life < 3.6e-4] = 3.6e-4
    return life


def schedule(star_ages, particle_type, mass):
    """drv:244, 339-341 on whole arrays, as the driver evaluates them -> (supernova_pos, max_rel_age, max star mass in
    solar masses)."""
    ages = np.asarray(star_ages, dtype=np.float64); m = np.asarray(mass, dtype=np.float64)
    pt = np.asarray(particle_type, dtype=np.float64)
    with np.errstate(all="ignore"):
        rel = ages / lifetime(m / SOLAR_MASS) / (YEAR * 1e10)
        return np.where(rel > 1.)[0], float(np.max(rel)), float(np.max(m[pt == 1] / SOLAR_MASS))


def select(particle_type, ptype, mass=None, window=None):
    """The indices a selection returns: ascending, the type's rows, with a window lo < mass / solar_mass < hi."""
    pt = np.asarray(particle_type, dtype=np.float64)
    cond = pt == ptype
    if window is not None:
        u = np.asarray(mass, dtype=np.float64) / SOLAR_MASS
        with np.errstate(all="ignore"):
            cond = cond & (u > window[0]) & (u < window[1])
    return np.flatnonzero(cond)


def agb_outputs(mass, particle_type, f_un, star_ages, OVERALL_AGE, mu_specie):
    """drv:660-664 on whole arrays."""
    m = np.asarray(mass, dtype=np.float64); pt = np.asarray(particle_type, dtype=np.float64)
    f_un = np.asarray(f_un, dtype=np.float64); ages = np.asarray(star_ages, dtype=np.float64)
    cond = ((pt == 1) & (m / SOLAR_MASS > 1.) & (m / SOLAR_MASS < 7.))
    with np.errstate(all="ignore"):
        return dict(AGB_condition=cond, AGB_list=m[cond],
                    AGB_time_until=lifetime(m[cond] / SOLAR_MASS) * 1e10 * YEAR - ages[cond] + OVERALL_AGE,
                    AGB_metallicity=np.sum((f_un * mu_specie)[cond].T[6:], axis=0) / np.sum((f_un * mu_specie)[cond], axis=1),
                    AGB_composition=((f_un * mu_specie)[cond].T / np.sum((f_un * mu_specie)[cond], axis=1)).T)


def make_state(seed, n, S, mix="all"):
    """Seeded arrays of a census: mix in {"all", "no_star", "no_dust", "all_dust"}."""
    rng = np.random.RandomState(seed)
    probs = {"all": [0.6, 0.15, 0.25], "no_star": [0.7, 0.0, 0.3], "no_dust": [0.8, 0.2, 0.0], "all_dust": [0.0, 0.0, 1.0]}[mix]
    pt = rng.choice([0., 1., 2.], size=n, p=probs)
    m = np.exp(rng.uniform(np.log(0.05), np.log(20.0), size=n)) * SOLAR_MASS
    f = rng.rand(n, S) + 1e-3
    mus = MU_SPECIE[np.arange(S) % MU_SPECIE.shape[0]] * (1.0 + 0.01 * (np.arange(S) // MU_SPECIE.shape[0]))
    return dict(mass=m, particle_type=pt, f_un=f, mu_specie=mus, velocities=rng.normal(size=(n, 3)) * 2e4,
                total_accel=rng.normal(size=(n, 3)) * 1e-9, E_internal=np.exp(rng.normal(size=n)) * 1e40,
                T=np.exp(rng.uniform(np.log(3.), np.log(1e4), size=n)),
                star_ages=np.where(pt == 1, rng.uniform(0., 3e10, size=n) * YEAR, -1.0))
