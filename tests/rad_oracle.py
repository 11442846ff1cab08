"""NumPy restatement of the radiative transfer of the reference's rad_heating (nsc:922-965) - the yardstick of the
rad_* tests.  Written from the formulas, not from the reference's text.

With C2 = 3 pi / 80 (nsc:48), particles p (all types) at x_p with h_p = sizes, m_p, mu_p, sigma_p = cross_array, sources
a_s and targets b_q, u = b_q - a_s:

    w_p              = C2 h_p^-2 sigma_p m_p / (mu_p amu)
    d2_p             = |(x_p - a_s) x u|^2 / |u|^2                      the whole infinite line ("line")
    blocked[s,q]     = sum_p [d2_p < h_p^2] w_p                         ("segment": and 0 <= (x_p - a_s).u < |u|^2)
    star_distance    = |u|
    over the non-star particles g, in the caller's order:
    gd[q,g] = |x_g - b_q|,  sd2[s,g] = |x_g - a_s|
    lum_factor[s,g]  = nan_to_num(sd2 sum_q((gd + 1)^-2 / sd[s,q] blocked[s,q]) / sum_q (gd + 1)^-2)
    extinction[g]    = w_g,  a_int = pi h_g^2,  df = (nan_to_num(sd2)^2 + min(h over gas)^2) 4 pi
    l[s,g]           = nan_to_num(exp(-nan_to_num(lum_factor)) / df L_s a_int extinction)
    lf2[g]           = sum_s l dt solar_luminosity
    momentum[g]      = sum_s (x_g - a_s)/sd2 l / m_g dt / c

Error bounds (derived, not tuned).  TAU = 1e-12 is SURVEY 8c's bound for a sum evaluated in another order:
|x - ref| <= TAU sum|term|; ULPS = 16 ulp stands for the handful of correctly rounded operations around each sum.
  blocked        TAU * blocked (every term is non-negative, so sum|term| is the column itself)
  star_distance  4 ulp
  extinction     8 ulp (five operations, a power among them)
  lum_factor     a quotient of two sums of non-negative terms over q; the numerator's terms carry the column's
                 error: relative TAU (column) + TAU (numerator sum) + TAU (denominator sum) + ULPS
  l[s,g]         its exponent is lum_factor itself, so the ABSOLUTE error of lum_factor is the relative error of
                 l: b_l = l (lum_factor_bound + ULPS) - up to 170 x 3 TAU on the fixtures, not a flat rtol
  lf2            sum_s (b_l + TAU l) dt solar_luminosity
  momentum       per component sum_s |unit| (b_l + TAU l) / m dt / c
A column is a top-hat: a particle crossing d2 = h^2 changes it by a whole term.  Every comparison is therefore valid
only where no (particle, ray) pair is near an edge; `margin` is the smallest relative distance from one,
min |d2_p / h_p^2 - 1| over all pairs (segment mode: also |t|, |t - 1| of the foot point t = (x_p - a).u / |u|^2 for
the pairs inside the cylinder - but for a particle that IS the ray's source or target, bit for bit: its test is
decided exactly, the source end in, the target end out).  A caller checks margin > 1e-9 before trusting a comparison.
"""
import numpy as np

C2 = 3 * np.pi / 80
AMU = 1.66053906892e-27
SOLAR_LUMINOSITY = 3.846e26
C_LIGHT = 299792458.0
EPS = 2.0 ** -52
TAU = 1e-12
ULPS = 16 * EPS
MODES = ("line", "segment")


def weights(sizes, masses, mu, cross, amu=AMU):
    h = np.asarray(sizes, dtype=np.float64)
    with np.errstate(all="ignore"):
        return C2 * h ** -2.0 * np.asarray(cross, dtype=np.float64) * np.asarray(masses, dtype=np.float64) / \
            (np.asarray(mu, dtype=np.float64) * amu)


def columns(positions, sizes, masses, mu, cross, sources, targets, mode="line", amu=AMU):
    """-> dict: blocked, star_distance (n_src, n_dst), their bounds, margin (inf without any pair), w (n,)."""
    if mode not in MODES:
        raise ValueError("mode must be 'line' or 'segment'")
    x = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    a = np.asarray(sources, dtype=np.float64).reshape(-1, 3)
    b = np.asarray(targets, dtype=np.float64).reshape(-1, 3)
    h2 = np.asarray(sizes, dtype=np.float64) ** 2
    w = weights(sizes, masses, mu, cross, amu)
    blocked = np.zeros((a.shape[0], b.shape[0]))
    sd = np.zeros((a.shape[0], b.shape[0]))
    margin = np.inf
    with np.errstate(all="ignore"):
        for s in range(a.shape[0]):
            rel = x - a[s]
            for q in range(b.shape[0]):
                u = b[q] - a[s]
                uu = np.sum(u ** 2)
                d2 = np.sum(np.cross(rel, u) ** 2, axis=1) / uu
                inside = d2 < h2
                edge = np.abs(d2 / h2 - 1.0)
                if mode == "segment":
                    # foot point: both sides of "t < |u|^2" by the same three operations, so a particle AT the target
                    # gives equality bit for bit (out: half-open) and one AT the source gives 0 exactly (in)
                    t = rel[:, 0] * u[0] + rel[:, 1] * u[1] + rel[:, 2] * u[2]
                    tu = u[0] * u[0] + u[1] * u[1] + u[2] * u[2]
                    at_end = np.all(rel == 0.0, axis=1) | np.all(rel == u, axis=1)
                    near = inside & ~at_end
                    ends = np.concatenate([np.abs(t[near] / tu), np.abs(t[near] / tu - 1.0)])
                    edge = np.concatenate([edge, ends])
                    inside = inside & (t >= 0.0) & (t < tu)
                edge = edge[~np.isnan(edge)]
                if edge.size:
                    margin = min(margin, float(edge.min()))
                blocked[s, q] = np.sum(w[inside])
                sd[s, q] = uu ** 0.5
    return dict(blocked=blocked, star_distance=sd, blocked_bound=TAU * np.abs(blocked),
                star_distance_bound=4 * EPS * sd, margin=margin, w=w)


def _finite(a):
    return np.where(np.isfinite(a), a, 0.0)


def transfer(positions, ptypes, masses, sizes, cross, mu, sources, luminosities, targets, dt, mode="line", amu=AMU,
             solar_luminosity=SOLAR_LUMINOSITY, c=C_LIGHT):
    """-> dict: lf2 (G,), momentum (G, 3), extinction (G,), blocked, star_distance (n_src, n_dst), lum_factor (n_src, G),
    "<name>_bound" for each, and margin; G = the particles with ptypes != 1.  ValueError without a gas particle."""
    x = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    pt = np.asarray(ptypes, dtype=np.float64)
    m = np.asarray(masses, dtype=np.float64)
    h = np.asarray(sizes, dtype=np.float64)
    a = np.asarray(sources, dtype=np.float64).reshape(-1, 3)
    b = np.asarray(targets, dtype=np.float64).reshape(-1, 3)
    L = np.asarray(luminosities, dtype=np.float64).reshape(-1)
    if not (pt == 0).any():
        raise ValueError("no particle with ptypes == 0")
    col = columns(x, h, m, mu, cross, a, b, mode, amu)
    blocked, sd = col["blocked"], col["star_distance"]
    gas = pt != 1
    xg, hg, mg = x[gas], h[gas], m[gas]
    G, S = xg.shape[0], a.shape[0]
    with np.errstate(all="ignore"):
        gd = np.sqrt(np.sum((xg[None, :, :] - b[:, None, :]) ** 2, axis=2))              # (n_dst, G)
        rel = xg[None, :, :] - a[:, None, :]                                            # (S, G, 3)
        sd2 = np.sqrt(np.sum(rel ** 2, axis=2))
        wq = (gd + 1.0) ** -2.0
        den = np.sum(wq, axis=0)
        lum = np.zeros((S, G))
        for s in range(S):
            lum[s] = np.nan_to_num(sd2[s] * np.sum((wq.T / sd[s] * blocked[s]).T, axis=0) / den)
        ext = col["w"][gas]
        a_int = np.pi * hg ** 2
        df = (np.nan_to_num(sd2) ** 2 + np.min(h[pt == 0]) ** 2) * 4.0 * np.pi
        ell = np.nan_to_num(((np.exp(-np.nan_to_num(lum)) / df).T * L).T * a_int * ext)
        lf2 = np.sum(ell, axis=0) * dt * solar_luminosity
        unit = rel / sd2[:, :, None]
        mom = (np.sum(unit * ell[:, :, None], axis=0) / mg[:, None]) * dt / c
        lum_b = np.abs(lum) * (3 * TAU + ULPS)
        ell_b = np.abs(ell) * (lum_b + ULPS) + TAU * np.abs(ell)
        lf2_b = np.sum(_finite(ell_b), axis=0) * dt * solar_luminosity
        mom_b = np.sum(_finite(np.abs(unit) * ell_b[:, :, None]), axis=0) / np.abs(mg[:, None]) * dt / c
    return dict(lf2=lf2, momentum=mom, extinction=ext, blocked=blocked, star_distance=sd, lum_factor=lum,
                lf2_bound=_finite(lf2_b), momentum_bound=_finite(mom_b), extinction_bound=8 * EPS * np.abs(ext),
                blocked_bound=col["blocked_bound"], star_distance_bound=col["star_distance_bound"],
                lum_factor_bound=_finite(lum_b), margin=col["margin"])


OUTPUTS = ("lf2", "momentum", "extinction", "blocked", "star_distance", "lum_factor")


def assert_within(name, x, ref, bound, what=""):
    """|x - ref| <= bound elementwise, no element left out; NaN must match NaN, inf the same inf."""
    x, ref, bound = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert x.shape == ref.shape, (what, name, x.shape, ref.shape)
    ok = (np.isnan(x) & np.isnan(ref)) | (x == ref)
    with np.errstate(invalid="ignore"):
        ok |= np.abs(x - ref) <= bound
    if not ok.all():
        bad = np.argwhere(~ok)
        rel = np.abs(x - ref)[~ok] / np.maximum(np.broadcast_to(bound, x.shape)[~ok], 1e-300)
        w = tuple(bad[np.argmax(rel)])
        raise AssertionError("%s %s: %d of %d elements beyond the bound; worst at %s: got %r, ref %r, |diff| %.3e, bound %.3e"
                             % (what, name, len(bad), x.size, w, x[w], ref[w], abs(x[w] - ref[w]),
                                np.broadcast_to(bound, x.shape)[w]))


def worst_ratio(x, ref, scale):
    """max |x - ref| / scale over the elements with a positive finite scale (for the figures a test prints)."""
    x, ref, scale = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.asarray(scale, dtype=np.float64)
    with np.errstate(all="ignore"):
        r = np.abs(x - ref) / scale
    r = r[np.isfinite(r)]
    return float(r.max()) if r.size else 0.0
