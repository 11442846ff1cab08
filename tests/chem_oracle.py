"""NumPy restatement of the reference's chemisputtering_2 (nsc:1265-1416) - the yardstick of the chem_* tests.  Written
from the formulas (include/sphx.h, sphx_chemisputtering_2), not from the reference's text.

Three parts:
  rows()    what a dust row j forms from the INPUTS alone (any order): the gas weights w = Weigh2 / mu of its list
            entries, whether it contributes (a gas entry, and sum w > 0), the SPH composition density, the temperature,
            F_sput, new0 = (F_sput - 1) num0[j] and the reuptake weight wk of every entry (one number per entry: the
            same for every column >= 6, zero below).
  sweep()   the ordered part, with np.longdouble where the reference has it.  Rows in ascending j; a row's first-stage
            losses new0 wk are clamped against the counts of its list entries as they stand (clamp 1:
            num - loss < 0.01 num -> 0.99 num; clamp 2: num < 0 -> num; both on EVERY list entry, a dust or star entry
            or the row itself included, where the loss is 0 and only a negative count acts), summed in list order,
            clamped against the row's own count (clamp 3), spread again by wk, subtracted from the entries and added to
            the row.  `deposits=None` is the reference's order: a row sees what the earlier rows left.  With
            `deposits=(sumc, new2)` the counts a row sees are formed from the GIVEN clamped sums of the earlier rows
            instead - one round of the library's iteration.
  rounds()  iterates sweep from the unclamped sums until a round changes no bit.  A row whose earlier sharers have their
            sequential value gets its sequential value, so by induction over the depth of the sharing graph the fixed
            point is the sequential result, bit for bit; at most (contributing rows + 1) rounds.
  sputter() = rows + sweep (sequential) + the closing correction of negative counts, mass_new, f_un_new.

Entries outside [0, N) contribute nothing.  A list row is taken to hold distinct indices.  A non-gas entry's weight is 0
(the reference multiplies by False: NaN data of a non-gas entry would give NaN there); a gas entry's weight is
v (v > 0) as written, NaN staying NaN.

Error bounds: every output comes with a first-order "<name>_bound", derived, not tuned, the way dust_oracle derives its
own.  EPS = 2^-52, TAU = 1e-12 sum|term| for every sum that may be evaluated in another order or precision (the library
adds in double and in list order where NumPy adds pairwise or in longdouble), ULPS = 16 EPS for the handful of rounded
operations around each coefficient.
  W = c q^3 / (64 pi d^9), q = (m/m_0)^(2/3) d^2 - r^2 cancels near the edge of the support: dq = 4 EPS (h2 + r2) + ULPS h2,
  dW = 3 |c| q^2 dq / (64 pi d^9) + ULPS |W|, absolute, valid through q = 0.
  exp(x) carries (dx + ULPS) exp(x).  F_sput - 1 = a (E - 1) / L_u with a = composition density - sput_y: the inputs'
  bounds go through this form to first order, the roundings of K_u, L_u and the quotient act on F_sput itself (absolute).
  min / max (the yields' limits, sput_y against dust_composition, the 0.01 floor) are 1-Lipschitz: the bound passes
  through, and is 0 where the limit holds by more than the bound.
  In the sweep every count carries the bounds of what was subtracted from it; a clamped loss carries 0.99 of the
  count's bound (clamp 1, 3) or the count's (clamp 2) - and since that loss returns to the same count through wk, the
  count's own bound passes with the factor |1 - alpha wk| (alpha = 0.99 or 1), which is what keeps a count that is taken
  down to 1 % again and again (tests: the hub) at a relative bound.
Decisions: the three clamps, the limits of Y_H and Y_He, sput_y > dust_composition, F < 0.01, w > 0, the 1e-15 branch of
the reuptake weight, and neg_comps < 0 per column ("sign").  Which of the two sums of the closing correction a count
enters is no decision of its own: the sums, the zeroing and the rescale are continuous in every count through 0, and a
count within its bound of 0 adds its bound to both sums'.  `slack` is, per kind, the smallest ratio of a decision's margin to the bound's size at that decision; a
decision between exact values (both sides' bounds 0, e.g. 0 < 0) cannot fall the other way and is left out.  A slack of
1e6 or more means the library decides as the restatement does: the counts are then equal and no element needs leaving
out of a comparison.
"""
import numpy as np

EPS = 2.0 ** -52
TAU = 1e-12
ULPS = 16 * EPS
LD = np.longdouble
K_B = 1.380649e-23
AMU = 1.66053906892e-27
SOLAR_MASS = 1.989e30
M_0 = 10 ** 1.5 * SOLAR_MASS
DT_0 = 60. * 60. * 24. * 365. * 250000.
MU_SPECIE = np.array([2.0158, 4.0026, 1.0079, 1.0074, 4.0021, 4.0016, 0.0005, 140.69, 60.08, 12.0107, 28.0855, 55.834,
                      100.39, 131.93, 40.096])
MINERAL_DENSITIES = np.array([1.e19, 1e19, 1e19, 1e19, 1e19, 1e19, 1e19, 3320, 2260, 2266, 2329, 7870, 3250, 3250., 3166.])
SPUTTERING_YIELDS = np.array([0, 0, 0, 0, 0, 0, 0, 0.137, 0.295, 0.137, 0.295, 0.137, 0.137, 0.137, 0.137])
MRN = np.array([50e-10, 5000e-10])
FIRST = 6                       # columns below are refractory to chemisputtering: F = 1, reuptake weight 0
OUTPUTS = ("mass_new", "f_un_new")
COUNTS = ("rows", "pairs", "clamp1", "clamp2", "clamp3", "columns_corrected", "rounds")
DECISIONS = ("clamp1", "clamp2", "clamp3", "yield", "select", "floor", "weight", "branch", "sign")


def tables(S, mu_specie=None, mineral_densities=None, sputtering_yields=None):
    """The per-species tables of length S: the reference's 15 entries, cut or continued (mu 50, density 3000, yield
    0.137) where S is not 15 and none is given."""
    out = []
    for given, dflt, more in ((mu_specie, MU_SPECIE, 50.0), (mineral_densities, MINERAL_DENSITIES, 3000.0),
                              (sputtering_yields, SPUTTERING_YIELDS, 0.137)):
        if given is None:
            given = np.concatenate([dflt, np.full(max(0, S - len(dflt)), more)])[:S]
        given = np.ascontiguousarray(given, dtype=np.float64)
        assert given.shape == (S,)
        out.append(given)
    return tuple(out)


def _fin(a):
    return np.where(np.isfinite(a), a, 0.0)


def _seq(a):
    """Sum along axis 1 in list order (np.sum adds a contiguous axis pairwise)."""
    return np.cumsum(a, axis=1)[:, -1]


def _slack(margin, bound):
    """min margin / bound over the decisions that CAN fall the other way (bound > 0) -> float (inf if none)."""
    margin, bound = np.broadcast_arrays(np.asarray(margin, dtype=np.float64), np.asarray(bound, dtype=np.float64))
    live = (bound > 0) & np.isfinite(margin)
    return float(np.min(margin[live] / bound[live])) if live.any() else np.inf


def rows(points, neighbor, mass, f_un, mu_array, sizes, T, particle_type, d, dt, mu_specie=None, mineral_densities=None,
         sputtering_yields=None, mrn=MRN, k_B=K_B, amu=AMU, m_0=M_0):
    """The order-independent part -> dict: num0, num0_b (N,S); dust (the dust rows), contributes (per dust row);
    valid, gas (nd,K); w (gas weights), wk, wk_b (nd,K); F, new0, new0_b (nd,S); T_sph; slack (dict)."""
    x = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = x.shape[0]
    nb = np.asarray(neighbor, dtype=np.int64)
    m, mu, T, pt = (np.asarray(a, dtype=np.float64) for a in (mass, mu_array, T, particle_type))
    f = np.asarray(f_un, dtype=np.float64)
    S = f.shape[1]
    assert S > FIRST
    mus, dens, ys = tables(S, mu_specie, mineral_densities, sputtering_yields)
    mrn = np.asarray(mrn, dtype=np.float64)
    slack = dict.fromkeys(("yield", "select", "floor", "weight", "branch"), np.inf)
    with np.errstate(all="ignore"):
        mubase = np.sum(f * mus, axis=1)
        num0 = (f.T * m / mubase).T
        num0_b = np.abs(num0) * (TAU * _fin(np.sum(np.abs(f * mus), axis=1) / np.abs(mubase))[:, None] + ULPS)
        num0_b = np.where(num0 == 0.0, 0.0, _fin(num0_b))
        dust = np.nonzero(pt == 2)[0]
        nd = len(dust)
        nbd = nb[dust]
        valid = (nbd >= 0) & (nbd < n)
        p = np.where(valid, nbd, 0)
        gas = valid & (pt[p] == 0)
        # Weigh2 of every entry (nsc:673-676) and its bound
        h2 = (m / m_0) ** (2. / 3.) * d ** 2
        c = m * 315 * (m_0 / m) ** 3
        den = 64 * np.pi * d ** 9
        r2 = np.sum((x[p] - x[dust][:, None, :]) ** 2, axis=2)
        q = h2[p] - r2
        W = c[p] * q ** 3 / den
        W_b = _fin(3 * np.abs(c[p]) * q ** 2 * (4 * EPS * (h2[p] + r2) + ULPS * h2[p]) / den + ULPS * np.abs(W))
        v = W / mu[p]
        w = np.where(gas, v * (v > 0), 0.0)
        w_b = np.where(gas & (v > 0), _fin(W_b / np.abs(mu[p])) + ULPS * np.abs(w), 0.0)
        slack["weight"] = _slack((np.abs(q) / (h2[p] + r2))[gas], 4 * EPS + ULPS)
        sw = np.sum(w, axis=1)
        contributes = np.any(gas, axis=1) & (sw > 0)
        sw_b = np.sum(w_b, axis=1) + TAU * np.sum(np.abs(w), axis=1)
        Tl = np.where(pt[p] == 1, 2.73, T[p])
        swT = np.sum(w * Tl, axis=1)
        T_sph = swT / sw
        relT = _fin((np.sum(w_b * np.abs(Tl), axis=1) + TAU * np.sum(np.abs(w * Tl), axis=1)) / np.abs(swT) + sw_b / np.abs(sw)) + ULPS
        wf = w[:, :, None] * f[p]                                            # (nd,K,S)
        # (the reference sums a transposed product: NumPy adds its contiguous axis, k, pairwise)
        scd = np.sum(np.ascontiguousarray(wf.transpose(0, 2, 1)), axis=2) * mus
        scd_b = (np.sum(w_b[:, :, None] * np.abs(f[p]), axis=1) + TAU * np.sum(np.abs(wf), axis=1)) * mus + ULPS * np.abs(scd)
        self_w2d = m[dust] * 315 * (sizes[dust] ** 2 - 0.0) ** 3 / (64 * np.pi * sizes[dust] ** 9)
        dc = self_w2d[:, None] * f[dust] * mus
        dc_b = ULPS * np.abs(dc)
        J0 = -np.diff(mrn ** -0.5) / np.diff(mrn ** 0.5) / (3 * dens)
        J = J0 * (k_B * T_sph[:, None] / (2 * np.pi * mus * amu)) ** 0.5
        relJ = (0.5 * relT + ULPS)[:, None]
        e = np.exp(-4600 / T_sph)
        e_b = e * (np.abs(4600 / T_sph) * relT + ULPS)
        Y, Y_b = [], []
        for a, lo, hi in ((0.5, 1e-7, 1e-3), (5, 1e-6, 1e-2)):
            y, y_b = a * e, a * e_b
            for lim in (lo, hi):
                slack["yield"] = min(slack["yield"], _slack(np.abs(y - lim)[contributes], y_b[contributes]))
            yc = np.where(lo > y, lo, y)
            yc = np.where(hi < yc, hi, yc)
            y_b = np.where((y + y_b < lo) | (y - y_b > hi), 0.0, y_b)
            Y.append(yc[:, None] * ys / np.max(ys)); Y_b.append(y_b[:, None] * ys / np.max(ys) + ULPS * np.abs(Y[-1]))
        t3, t4 = scd[:, 3:4] / mus[3], scd[:, 4:5]
        sput = (t3 * Y[0] + t4 * Y[1] / mus[4]) * mus
        sput_b = ((scd_b[:, 3:4] / mus[3] * Y[0] + np.abs(t3) * Y_b[0] + (scd_b[:, 4:5] * Y[1] + np.abs(t4) * Y_b[1]) / mus[4]) * mus
                  + ULPS * np.abs(sput))
        live = contributes[:, None] & np.ones(S, bool)[None, :] & (np.arange(S) >= FIRST)[None, :]
        slack["select"] = _slack(np.abs(sput - dc)[live], (sput_b + dc_b)[live])
        sel = sput > dc
        sput_b = np.where(sel, dc_b, sput_b)
        sput = np.where(sel, dc, sput)
        Ku = scd + dc - sput
        Ku_b = scd_b + dc_b + sput_b + ULPS * (np.abs(scd) + np.abs(dc) + np.abs(sput))
        xx = Ku * J * dt
        xx_b = Ku_b * np.abs(J * dt) + np.abs(xx) * (relJ + ULPS)
        E = np.exp(xx)
        E_b = E * (xx_b + ULPS)
        Lu = scd + dc * E - sput
        Lu_b = scd_b + dc_b * E + np.abs(dc) * E_b + sput_b + ULPS * (np.abs(scd) + np.abs(dc * E) + np.abs(sput))
        F = Ku / Lu
        F = F * E
        # F - 1 = a (E - 1) / L with a = scd - sput: what the inputs' bounds do to F goes through THIS form (a common
        # relative error of the weights moves F - 1 by that fraction of F - 1, not of F); the roundings of K, L and the
        # quotient act on F itself
        a_, Em1 = scd - sput, np.expm1(xx)
        F_b = ((np.abs(Em1) * (scd_b + sput_b) + np.abs(a_) * E_b) / np.abs(Lu) + np.abs(a_ * Em1 / Lu) * (Lu_b / np.abs(Lu))
               + ULPS * np.abs(F) * (1 + (np.abs(scd) + np.abs(dc * E) + np.abs(sput)) / np.abs(Lu)))
        nanF = np.isnan(F)
        F = np.where(nanF, 1.0, F)
        F_b = np.where(nanF, 0.0, F_b)
        slack["floor"] = _slack(np.abs(F - 0.01)[live], F_b[live])
        F_b = np.where(F + F_b < 0.01, 0.0, F_b)
        F = np.where(F < 0.01, 0.01, F)
        F[:, :FIRST] = 1.0; F_b[:, :FIRST] = 0.0
        F_b = np.where(np.isfinite(F_b), F_b, np.inf)
        new0 = (F - 1.) * num0[dust]
        new0_b = F_b * np.abs(num0[dust]) + np.abs(F - 1.) * num0_b[dust] + ULPS * np.abs(new0)
        # the reuptake weight: one number per entry (nsc:1336-1363)
        rp = gas & (w > 0)
        rl = np.sum(rp, axis=1)
        rw0 = np.where(rp, w * f[p][:, :, 5] * mus[5], 0.0)
        rw0_b = np.where(rp, w_b * np.abs(f[p][:, :, 5]) * mus[5] + ULPS * np.abs(rw0), 0.0)
        A = _seq(rw0)[:, None]
        A_b = (np.sum(rw0_b, axis=1) + TAU * np.sum(np.abs(rw0), axis=1))[:, None]
        a1 = rw0 / A
        a2 = a1 / _seq(np.where(rp, a1, 0.0))[:, None]
        tot = (S - FIRST) * np.sum(np.where(rp, np.nan_to_num(a2), 0.0), axis=1)
        slack["branch"] = _slack(np.abs(tot - 1e-15)[contributes], (TAU * np.abs(tot) + _fin(A_b[:, 0] / np.abs(A[:, 0])))[contributes])
        fill = np.where(tot < 1e-15, 1. / rl, 0.0)[:, None]
        a3 = np.where(np.isnan(a2), fill, a2)
        wk = np.nan_to_num(a3 / _seq(np.where(rp, a3, 0.0))[:, None])
        wk = np.where(rp, wk, 0.0)
        wk_b = np.where(np.isnan(a2), ULPS * np.abs(wk), _fin(rw0_b / np.abs(A)) + np.abs(wk) * (_fin(A_b / np.abs(A)) + 3 * (TAU + ULPS)))
        wk_b = np.where(rp, wk_b, 0.0)
    return dict(n=n, S=S, mus=mus, num0=num0, num0_b=num0_b, dust=dust, contributes=contributes, nb=nbd, valid=valid, gas=gas,
                w=w, wk=wk, wk_b=wk_b, F=F, F_b=F_b, new0=new0, new0_b=new0_b, T_sph=T_sph, scd=scd, dc=dc, sput=sput, x=xx, slack=slack)


def sweep(R, deposits=None, bounds=True):
    """One pass over the contributing rows in ascending j -> dict: num (N,S) (double, as the reference keeps it), num_b,
    sumc, new2 (nd,S) (longdouble: the clamped sum and what the row itself receives), counts, slack."""
    S = R["S"]
    num = R["num0"].copy()
    num_b = R["num0_b"].copy()
    nd = len(R["dust"])
    sumc = np.zeros((nd, S), dtype=LD); new2 = np.zeros((nd, S), dtype=LD)
    cnt = dict(clamp1=0, clamp2=0, clamp3=0)
    slack = dict(clamp1=np.inf, clamp2=np.inf, clamp3=np.inf)
    hi = np.arange(S) >= FIRST
    with np.errstate(all="ignore"):
        for a in np.nonzero(R["contributes"])[0]:
            j = R["dust"][a]
            ks = np.nonzero(R["valid"][a])[0]
            idx = R["nb"][a, ks]
            rw = np.zeros((len(ks), S)); rw[:, FIRST:] = R["wk"][a, ks][:, None]
            rw_b = np.zeros((len(ks), S)); rw_b[:, FIRST:] = R["wk_b"][a, ks][:, None]
            rw = rw.astype(LD)
            new = R["new0"][a].astype(LD)
            loss = new * rw
            loss_b = R["new0_b"][a] * np.abs(rw) + np.abs(new) * rw_b + ULPS * np.abs(loss)
            cur, cur_b = num[idx], num_b[idx]
            lhs = cur - loss - 0.01 * cur
            c1 = cur - loss < 0.01 * cur
            c2 = cur < 0
            if bounds:
                slack["clamp1"] = min(slack["clamp1"], _slack(np.abs(lhs)[:, hi], (1.01 * cur_b + loss_b)[:, hi].astype(np.float64)))
                slack["clamp2"] = min(slack["clamp2"], _slack(np.abs(cur)[:, hi], cur_b[:, hi]))
            cnt["clamp1"] += int(np.count_nonzero(c1[:, hi])); cnt["clamp2"] += int(np.count_nonzero(c2[:, hi]))
            loss[c1] = (0.99 * cur)[c1]
            loss[c2] = cur[c2]
            loss_b = np.where(c2, cur_b, np.where(c1, 0.99 * cur_b + ULPS * np.abs(cur), loss_b))
            tot = np.sum(loss, axis=0)
            tot_b = np.sum(loss_b, axis=0) + TAU * np.sum(np.abs(_fin(loss.astype(np.float64))), axis=0)
            own, own_b = num[j], num_b[j]
            c3 = tot + own < 0.01 * own
            if bounds:
                slack["clamp3"] = min(slack["clamp3"], _slack(np.abs(tot + own - 0.01 * own)[hi], (tot_b + 1.01 * own_b)[hi].astype(np.float64)))
            cnt["clamp3"] += int(np.count_nonzero(c3[hi]))
            tot[c3] = -0.99 * own[c3]
            tot_b = np.where(c3, 0.99 * own_b + ULPS * np.abs(own), tot_b)
            loss = tot * rw
            got = np.sum(np.nan_to_num(loss), axis=0)
            sumc[a], new2[a] = tot, got
            if deposits is not None:                                         # what the LATER rows see: the given sums
                tot = deposits[0][a]
                loss = tot * rw
                got = deposits[1][a]
            loss_b = tot_b * np.abs(rw) + np.abs(tot) * rw_b + ULPS * np.abs(loss)
            got_b = np.sum(loss_b, axis=0) + TAU * np.sum(np.abs(_fin(loss.astype(np.float64))), axis=0)
            num[idx] = (num[idx] + np.nan_to_num(-loss)).astype(np.float64)
            num[j] = (num[j] + got).astype(np.float64)
            # a clamped loss IS a multiple of the entry's count (0.99 of it, or all of it), and it comes back through wk:
            # the count's own bound passes with the factor |1 - alpha wk|, not 1 + alpha wk
            alpha = np.where(c2, 1.0, np.where(c1, 0.99, 0.0)) * ~c3[None, :]
            others = np.maximum(tot_b[None, :] - alpha * cur_b, 0.0).astype(np.float64)
            dep = np.abs(_fin(loss.astype(np.float64)))
            num_b[idx] = (np.abs(1.0 - alpha * rw.astype(np.float64)) * cur_b + np.abs(rw.astype(np.float64)) * others
                          + np.abs(_fin(tot.astype(np.float64))) * rw_b + ULPS * (np.abs(cur) + dep))
            num_b[j] = num_b[j] + _fin(got_b.astype(np.float64)) + ULPS * np.abs(num[j])
    return dict(num=num, num_b=num_b, sumc=sumc, new2=new2, counts=cnt, slack=slack)


def _same_bits(a, b):
    return np.array_equal(a, b) or bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def rounds(R):
    """The library's iteration -> (the last round's sweep, the number of rounds).  Round 0 takes the unclamped sums."""
    with np.errstate(all="ignore"):
        prev = (R["new0"].astype(LD), R["new0"].astype(LD))
    limit = int(np.count_nonzero(R["contributes"])) + 1
    r = 0
    while True:
        out = sweep(R, deposits=prev, bounds=False)
        r += 1
        if (_same_bits(out["sumc"], prev[0]) and _same_bits(out["new2"], prev[1])) or r >= limit:
            return out, r
        prev = (out["sumc"], out["new2"])


def correct(num, num_b, mus):
    """The closing correction (nsc:1400-1409), mass_new, f_un_new and their bounds -> dict."""
    num = num.copy()
    num_b = num_b.copy()
    n, S = num.shape
    corrected = 0
    with np.errstate(all="ignore"):
        sign = np.inf
        for s in range(S):
            col, col_b = num[:, s], num_b[:, s]
            P, Ng = col > 0, col < 0
            pos, neg = np.sum(col[P]), np.sum(col[Ng])
            near = (np.abs(col) <= col_b) & (col_b > 0)                      # may sit on the other side of 0 in the library
            pos_b = np.sum(col_b[P | near]) + TAU * pos
            neg_b = np.sum(col_b[Ng | near]) + TAU * abs(neg)
            sign = min(sign, _slack(abs(neg), neg_b))
            if neg < 0:
                corrected += 1
                fac = 1. + neg / pos
                fac_b = neg_b / abs(pos) + abs(neg) * pos_b / pos ** 2 + ULPS * (1 + abs(neg / pos))
                col[Ng] = 0.; col_b[Ng] = 0.
                col_b[P] = col_b[P] * abs(fac) + np.abs(col[P]) * fac_b + ULPS * np.abs(col[P] * fac)
                col[P] *= fac
        mass_new = np.sum(num * mus, axis=1)
        mass_b = np.sum(num_b * mus, axis=1) + TAU * np.sum(np.abs(num * mus), axis=1)
        tot = np.sum(num, axis=1)
        tot_b = np.sum(num_b, axis=1) + TAU * np.sum(np.abs(num), axis=1)
        f_new = (num.T / tot).T
        f_b = num_b / np.abs(tot)[:, None] + np.abs(f_new) * (tot_b / np.abs(tot))[:, None] + ULPS * np.abs(f_new)
        f_b = np.where(np.isfinite(f_b), f_b, np.inf)
    return dict(mass_new=mass_new, f_un_new=f_new, mass_new_bound=mass_b, f_un_new_bound=f_b, columns_corrected=corrected, sign=sign)


def sputter(points, neighbor, mass, f_un, mu_array, sizes, T, particle_type, d, dt, model=False, **kw):
    """-> dict: mass_new (N,), f_un_new (N,S), "<name>_bound", counts (dict over COUNTS; `rounds` from the round model if
    model=True, else None), slack (dict over DECISIONS), contributes, num (the counts before the closing correction).
    model=True also asserts that the round model ends on the sequential result, bit for bit."""
    R = rows(points, neighbor, mass, f_un, mu_array, sizes, T, particle_type, d, dt, **kw)
    sq = sweep(R)
    nrounds = None
    if model:
        it, nrounds = rounds(R)
        assert _same_bits(it["num"], sq["num"]) and _same_bits(it["sumc"], sq["sumc"]) and _same_bits(it["new2"], sq["new2"])
        assert it["counts"] == sq["counts"]
    fin = correct(sq["num"], sq["num_b"], R["mus"])
    slack = dict(R["slack"], **sq["slack"])
    slack["sign"] = fin["sign"]
    counts = dict(rows=int(np.count_nonzero(R["contributes"])),
                  pairs=int(np.count_nonzero(R["gas"] & R["contributes"][:, None])), rounds=nrounds,
                  columns_corrected=fin["columns_corrected"], **sq["counts"])
    out = {nm: fin[nm] for nm in ("mass_new", "f_un_new", "mass_new_bound", "f_un_new_bound")}
    out.update(counts=counts, slack=slack, contributes=R["contributes"], dust=R["dust"], num=sq["num"], rows=R)
    return out


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
