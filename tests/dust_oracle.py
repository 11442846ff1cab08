"""NumPy restatement of the reference's supernova_destruction (nsc:1211-1263) - the yardstick of the dust_* tests.
Written from the formulas (include/sphx.h, sphx_supernova_destruction), not from the reference's text.

The pair term of (gas row j, dust entry i = neighbor[j,k]) is formed for all (N, K) at once; only the guard
    accept = (acc[i,t] + lost < limit_i);  lost *= accept;  acc[i,t] += lost
reads what earlier rows left, so the contributing rows are then walked in ascending j (inside a row all entries at once -
a row holds distinct indices; one that does not is walked entry by entry, a repeated index counting once per occurrence).
reup[j,t] adds the row's accepted losses in list order.  guard="count": limit = 1 (the reference's); guard="fraction":
limit = N_i (the library's own; the reference cannot produce it).  The selector `species_curve` has S entries of 0 (none),
1 (carbon), 2 (silicon); by default the reference's 14-entry tuple padded with 0.  Only (gas row, dust entry) pairs are
formed and an unselected species loses exactly 0, as in the library.  An entry outside [0, N) contributes nothing.

Error bounds: every output comes with a first-order "<name>_bound", derived, not tuned, the way cool_oracle derives its
own.  EPS = 2^-52.  TAU = 1e-12 sum|term| for every sum that may be evaluated in another order, ULPS = 16 EPS for the
handful of correctly rounded operations around each product or quotient (the project's figures): the
library forms q^3 and sizes^9 by multiplication where NumPy calls pow, and r^2, |dv|^2 left to right where NumPy's
reduction adds the first term last.
  wd = c q^3 / (64 pi s^9) with q = s^2 - r^2 cancels near the edge of the support: dq = 4 EPS (s^2 + r^2), so
  d wd = 3 |c| q^2 dq / (64 pi s^9) + ULPS |wd| - an ABSOLUTE bound, valid through q = 0, where the mask [wd > 0] may fall
  either way and rho is itself O(q^3).
  v = |dv| / 1000 carries ULPS v; the interpolant is piecewise linear, so d eff = L d v + ULPS |eff| with L the largest
  |slope| of the curve (its Lipschitz constant - valid across a knot); at the last knot the curve drops to 0, a decision
  (below).  ff = g eff ratio: relative errors add; the cap at 0.99 is 1-Lipschitz and a value further above it than its
  bound has bound 0.  lost = ff f N: d lost = d ff |f| N + ULPS |lost|.  The accepted losses are added in the same order
  by both, so acc and reup carry sum d lost + TAU sum |lost|; the final division adds ULPS.
Decisions: the guard, the cap, [wd > 0] and the ends of the knots are discrete.  `margins` returns for each the smallest
relative margin met - guard |acc + lost - limit| / limit, cap |ff - 0.99|, wd |q| / (s^2 + r^2), knots |v - v_end| / v_end -
and `slack`, the smallest ratio of a margin to the bound's relative size AT that decision ((d acc + d lost) / limit,
d ff, 4 EPS, ULPS).  A slack of 1e6 or more means no decision can fall the other way in the library: the regime counts
are then equal and no element needs leaving out of a comparison.
"""
import numpy as np

EPS = 2.0 ** -52
TAU = 1e-12
ULPS = 16 * EPS
CAP = 0.99
AMU = 1.66053906892e-27
SOLAR_MASS = 1.989e30
CRIT_MASS = 0.0001 * SOLAR_MASS
CRITICAL_DENSITY = 1000 * AMU * 10 ** 6
KNOTS_V = np.array([0., 50., 75., 100., 125., 150., 175., 200.])
KNOTS_C = np.array([0., 0.01, 0.04, 0.10, 0.18, 0.17, 0.18, 0.23])
KNOTS_SI = np.array([0., 0.02, 0.09, 0.23, 0.41, 0.40, 0.42, 0.40])
CURVES = (0, 0, 0, 0, 0, 0, 1, 2, 1, 2, 1, 1, 1, 0)
OUTPUTS = ("frac_destruction", "frac_reuptake")
COUNTS = ("lost", "accepted", "rejected", "rejected_by_accumulation", "capped")


def species_curve_default(S):
    return np.array((CURVES + (0,) * max(0, S - len(CURVES)))[:S], dtype=np.int32)


def _fin(a):
    return np.where(np.isfinite(a), a, 0.0)


def efficiency(v, knots_v, knots_y):
    """np.interp inside [v_0, v_7], 0 outside, NaN for NaN -> (eff, its Lipschitz constant)."""
    e = np.interp(v, knots_v, knots_y)
    e = np.where((v < knots_v[0]) | (v > knots_v[-1]), 0.0, e)
    return e, float(np.max(np.abs(np.diff(knots_y) / np.diff(knots_v))))


def destruction(points, velocities, neighbor, mass, f_un, mu_array, sizes, densities, particle_type, crit_mass=CRIT_MASS,
                critical_density=CRITICAL_DENSITY, species_curve=None, guard="count", amu=AMU, knots_v=KNOTS_V,
                knots_c=KNOTS_C, knots_si=KNOTS_SI):
    """-> dict: frac_destruction, frac_reuptake (N,S), "<name>_bound", counts (dict over COUNTS), contributes (N,),
    pairs (the number of (contributing row, dust entry) pairs), margins and slack (dicts over guard, cap, wd, knots; inf
    where no such decision was met)."""
    assert guard in ("count", "fraction")
    x = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    vel = np.asarray(velocities, dtype=np.float64).reshape(-1, 3)
    n = x.shape[0]
    nb = np.asarray(neighbor, dtype=np.int64)
    K = nb.shape[1]
    m, mu, s = (np.asarray(a, dtype=np.float64) for a in (mass, mu_array, sizes))
    dens, pt = np.asarray(densities, dtype=np.float64), np.asarray(particle_type, dtype=np.float64)
    f = np.asarray(f_un, dtype=np.float64)
    S = f.shape[1]
    sc = species_curve_default(S) if species_curve is None else np.asarray(species_curve, dtype=np.int32)
    assert sc.shape == (S,) and np.all((sc >= 0) & (sc <= 2))
    sel = np.nonzero(sc)[0]
    kv, kc, ks = (np.asarray(a, dtype=np.float64) for a in (knots_v, knots_c, knots_si))
    with np.errstate(all="ignore"):
        valid = (nb >= 0) & (nb < n)
        p = np.where(valid, nb, 0)
        pair = valid & (pt == 0)[:, None] & (pt[p] == 2)
        big = m > crit_mass
        s2 = s ** 2
        den = 64 * np.pi * s ** 9
        cw = np.where(big, m * 315, 0.0)
        w0 = m * 315 * (s2 - 0.0) ** 3 / den
        N = m / (mu * amu)
        r2 = np.sum((x[p] - x[:, None, :]) ** 2, axis=2)
        q = s2[p] - r2
        wd = cw[p] * q ** 3 / den[p]
        rho = np.where(pair, wd * (wd > 0), 0.0)
        wd_b = np.where(pair, _fin(3 * np.abs(cw[p]) * q ** 2 * (4 * EPS * (s2[p] + r2)) / den[p] + ULPS * np.abs(wd)), 0.0)
        contributes = np.any(pair & (rho > 0), axis=1) & ~np.any(pair & np.isnan(rho), axis=1)
        active = pair & contributes[:, None]
        v = np.sum((vel[p] - vel[:, None, :]) ** 2, axis=2) ** 0.5 / 1000.
        v_b = ULPS * np.abs(v)
        ratio = np.nan_to_num(rho / w0[p])
        ratio_b = _fin(wd_b / np.abs(w0[p])) + ULPS * np.abs(ratio)
        g = dens[:, None] * big[p] / critical_density
        eff = {}
        for code, ky in ((1, kc), (2, ks)):
            e, lip = efficiency(v, kv, ky)
            eff[code] = (e, lip * v_b + ULPS * np.abs(e))
        lost = np.zeros((n, K, S)); lost_b = np.zeros((n, K, S))
        ff_all = np.zeros((n, K, S)); ff_b_all = np.zeros((n, K, S))
        capped = np.zeros((n, K, S), dtype=bool)
        for t in sel:
            e, e_b = eff[int(sc[t])]
            ff = g * (e * ratio)
            ff_b = _fin(np.abs(g) * (e_b * np.abs(ratio) + np.abs(e) * ratio_b)) + ULPS * np.abs(ff)
            ff_all[:, :, t], ff_b_all[:, :, t] = np.where(active, ff, 0.0), np.where(active, ff_b, 0.0)
            cp = active & (ff >= CAP)
            capped[:, :, t] = cp
            ff_b = np.where(ff - ff_b > CAP, 0.0, ff_b)
            ff = np.where(cp, CAP, ff)
            lo = ff * f[p, t] * N[p]
            lost[:, :, t] = np.where(active, lo, 0.0)
            lost_b[:, :, t] = np.where(active, _fin(ff_b * np.abs(f[p, t]) * np.abs(N[p])) + ULPS * np.abs(_fin(lo)), 0.0)
        # ---- the guard, in ascending row order ----
        limit = N if guard == "fraction" else np.ones(n)
        acc = np.zeros((n, S)); acc_b = np.zeros((n, S))
        took = np.zeros((n, K, S)); took_b = np.zeros((n, K, S))
        cnt = dict.fromkeys(COUNTS, 0)
        cnt["capped"] = int(np.count_nonzero(capped))
        g_margin = g_slack = np.inf
        selm = np.zeros(S, dtype=bool); selm[sel] = True
        for j in np.nonzero(contributes)[0]:
            ks_ = np.nonzero(active[j])[0]
            groups = [ks_] if len(np.unique(p[j, ks_])) == len(ks_) else [ks_[a:a + 1] for a in range(len(ks_))]
            for kk in groups:
                idx = p[j, kk]
                L, Lb = lost[j, kk], lost_b[j, kk]
                lim = limit[idx][:, None]
                tot = acc[idx] + L
                accept = tot < lim
                live = selm[None, :] & ((L != 0) | (Lb != 0))
                if live.any():
                    mg = np.abs(tot - lim) / np.abs(lim)
                    rel = (acc_b[idx] + Lb) / np.abs(lim)
                    mg, rel = mg[live], rel[live]
                    ok = np.isfinite(mg)
                    if ok.any():
                        g_margin = min(g_margin, float(mg[ok].min()))
                        g_slack = min(g_slack, float((mg[ok] / np.maximum(rel[ok], 1e-300)).min()))
                pos = L > 0
                cnt["lost"] += int(np.count_nonzero(pos))
                cnt["accepted"] += int(np.count_nonzero(pos & accept))
                cnt["rejected"] += int(np.count_nonzero(pos & ~accept))
                cnt["rejected_by_accumulation"] += int(np.count_nonzero(pos & ~accept & (L < lim)))
                L2 = L * accept                                              # NaN x False = NaN
                Lb2 = np.where(accept, Lb + TAU * np.abs(_fin(L)), 0.0)
                acc[idx] += L2; acc_b[idx] += Lb2
                took[j, kk], took_b[j, kk] = L2, Lb2
        reup = np.zeros((n, S)); reup_b = np.zeros((n, S))
        for k in range(K):                                                   # list order
            reup = reup + took[:, k, :]; reup_b = reup_b + took_b[:, k, :]
        Nc = N[:, None]
        fd, fr = np.nan_to_num(acc / Nc), np.nan_to_num(reup / Nc)
        fd_b = _fin(acc_b / np.abs(Nc)) + ULPS * np.abs(fd)
        fr_b = _fin(reup_b / np.abs(Nc)) + ULPS * np.abs(fr)
        # ---- the other decisions' margins ----
        margins = dict(guard=g_margin); slack = dict(guard=g_slack)
        a3 = active[:, :, None] & selm[None, None, :]
        near = a3 & ((ff_all != 0) | (ff_b_all != 0))
        if near.any():
            mg = np.abs(ff_all - CAP)[near]
            margins["cap"] = float(mg.min()); slack["cap"] = float((mg / np.maximum(ff_b_all[near], 1e-300)).min())
        else:
            margins["cap"] = slack["cap"] = np.inf
        edge = pair & big[p]
        if edge.any():
            mg = (np.abs(q) / (s2[p] + r2))[edge]
            margins["wd"] = float(mg.min()); slack["wd"] = margins["wd"] / (4 * EPS)
        else:
            margins["wd"] = slack["wd"] = np.inf
        ends = [e for e in (kv[0], kv[-1]) if e != 0.0]
        if active.any() and ends:
            mg = min(float((np.abs(v - e) / abs(e))[active].min()) for e in ends)
            margins["knots"] = mg; slack["knots"] = mg / ULPS
        else:
            margins["knots"] = slack["knots"] = np.inf
    return dict(frac_destruction=fd, frac_reuptake=fr, frac_destruction_bound=fd_b, frac_reuptake_bound=fr_b, counts=cnt,
                contributes=contributes, pairs=int(np.count_nonzero(active)), margins=margins, slack=slack)


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
