"""NumPy restatement in longdouble of the elementwise half of the radiative block of the reference's time loop
(code_running.py:247-316 with nsc:976-1012) - the yardstick of the radiative-phase tests.  Written from the formulas
(include/sphx.h: sphx_rad_ionise, sphx_rad_heat_bookkeeping, sphx_rad_cool_bookkeeping), not from the driver's text.

    ionise            nsc:976-1012   -> f_un_new (N,S), frac_destroyed (G,3)
    heat_bookkeeping  drv:258-273    -> mu_array, gamma_array, cross_array, E_internal, T, totals, counts
    cool_bookkeeping  drv:283-311    -> the same and velocities

Every result comes with "<name>_bound", a per-element first-order bound on what an evaluation in double, with the sums
over species in another order, may differ by.  The bound is carried through the arithmetic by `V` (value, absolute error):
    an input                       exact (each stage is fed given arrays)
    a + b, a - b                   ea + eb + EPS |result|
    a b                            |a| eb + |b| ea + EPS |result|
    a / b                          ea / |b| + |a / b| eb / |b| + EPS |result|
    a sum over species             sum of the terms' errors + TAU sum |term|        (the project's bound for a re-ordered sum)
    exp(a)                         |result| (ea + TRANS),  TRANS = 16 ulp          (cool_oracle's allowance per transcendental)
    sqrt(a), a^(1/6)               |result| (ea / (2 |a|) + EPS), |result| (ea / (6 |a|) + TRANS)
    nan_to_num                     acts on the value rounded to float64; a NaN or an infinity it replaced is exact
    a clamp, min(max(a, lo), hi)   ea + e_lo + e_hi: continuous, so a comparison that falls the other way within the
                                   bound moves the result by no more than the bound; how many elements a clamp moved
                                   is therefore a range, counts[name] = (at least, at most): a star's E_internal, left at
                                   its limit by the heating, meets the cooling's limit again to within rounding
EPS = 2^-52 is one rounding; SUB, a few subnormal steps, is added to every error so that underflowing results compare.
Decisions that are not continuous: frac is set to 0 where atoms_total / amu < 1e-10 (the fixtures assert that no value
lies in (0, 1e-9)); the sign of a coefficient's quotient picks + 1 or exp (a quotient's sign is exact)."""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
TAU = 1e-12
TRANS = 16 * EPS
SUB = 4 * 5e-324
DMAX = np.finfo(np.float64).max
TOTALS = ("E_before", "E_after")
COUNTS = ("E_raised", "E_lowered", "T_raised", "T_lowered")


def _mulz(x, y):
    """x y with 0 where either factor is 0 (0 inf = 0: an exact operand carries no error whatever it is scaled by)."""
    with np.errstate(all="ignore"):
        return np.where((x == 0) | (y == 0), 0.0, x * y)


def _f(a):
    with np.errstate(all="ignore"):
        return np.abs(np.asarray(a)).astype(np.float64)


class V(object):
    """A longdouble array with a float64 absolute error bound per element."""

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, dtype=LD)
        self.e = np.zeros(self.v.shape) + np.asarray(e, dtype=np.float64)

    @staticmethod
    def of(x):
        return x if isinstance(x, V) else V(x)

    def _round(self, v, e):
        with np.errstate(all="ignore"):
            return V(v, np.nan_to_num(e, nan=np.inf) + EPS * np.nan_to_num(_f(v), nan=0.0) + SUB)

    def __add__(self, o):
        o = V.of(o)
        with np.errstate(all="ignore"):
            return self._round(self.v + o.v, self.e + o.e)
    __radd__ = __add__

    def __sub__(self, o):
        o = V.of(o)
        with np.errstate(all="ignore"):
            return self._round(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return V.of(o) - self

    def __neg__(self):
        return V(-self.v, self.e)

    def __mul__(self, o):
        o = V.of(o)
        with np.errstate(all="ignore"):
            return self._round(self.v * o.v, _mulz(_f(self.v), o.e) + _mulz(_f(o.v), self.e))
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = V.of(o)
        with np.errstate(all="ignore"):
            q = self.v / o.v
            inv = 1.0 / _f(o.v)
            return self._round(q, _mulz(self.e, inv) + _mulz(_mulz(_f(q), o.e), inv))

    def __rtruediv__(self, o):
        return V.of(o) / self

    def exp(self):
        with np.errstate(all="ignore"):
            r = np.exp(self.v)
            return V(r, _mulz(_f(r), self.e + TRANS) + SUB)

    def root(self, p, allowance):
        """self^(1/p)"""
        with np.errstate(all="ignore"):
            r = self.v ** (LD(1) / LD(p))
            return V(r, _mulz(_f(r), _mulz(self.e, 1.0 / (p * _f(self.v))) + allowance) + SUB)

    def nan_to_num(self):
        with np.errstate(all="ignore"):
            d = self.v.astype(np.float64)
            special = ~np.isfinite(d)
            return V(np.nan_to_num(d).astype(LD), np.where(special, 0.0, self.e))

    def where(self, cond, other):
        other = V.of(other)
        return V(np.where(cond, self.v, other.v), np.where(cond, self.e, other.e))

    def f64(self):
        return self.v.astype(np.float64)


def ssum(terms):
    """A sum over species of a list of V: the terms' errors plus TAU sum |term|."""
    with np.errstate(all="ignore"):
        v = sum(t.v for t in terms)
        e = sum(t.e for t in terms) + TAU * np.nan_to_num(sum(_f(t.v) for t in terms), nan=0.0)
    return V(v, e + SUB)


def _range(hit, tie):
    """How many elements a clamp moves: (at least, at most) - a comparison within its operands' bounds may fall either way."""
    return int(np.sum(hit & ~tie)), int(np.sum(hit | tie))


def clamp_low(a, lo):
    """a < lo -> lo"""
    with np.errstate(all="ignore"):
        hit = a.v < lo.v
        tie = (np.abs(a.v - lo.v).astype(np.float64) <= a.e + lo.e) & (a.e + lo.e > 0)      # (exact operands compare exactly)
    return V(np.where(hit, lo.v, a.v), a.e + lo.e), _range(hit, tie)


def clamp_high(a, hi, strict=True):
    with np.errstate(all="ignore"):
        hit = (a.v > hi.v) if strict else (a.v >= hi.v)
        tie = (np.abs(a.v - hi.v).astype(np.float64) <= a.e + hi.e) & (a.e + hi.e > 0)
    return V(np.where(hit, hi.v, a.v), a.e + hi.e), _range(hit, tie)


def _cols(f):
    return [V(f[:, t]) for t in range(f.shape[1])]


def ionise(f_un, ptypes, masses, lf2, frac_dest, photons_per_joule, mu_specie, cross_sections, amu):
    """-> dict: f_un_new (N,S), frac_destroyed (G,3) and their bounds."""
    f = np.asarray(f_un, dtype=np.float64)
    pt = np.asarray(ptypes, dtype=np.float64)
    n, S = f.shape
    ns = pt != 1
    g = f[ns]
    col = _cols(g)
    m = V(np.asarray(masses, dtype=np.float64)[ns])
    n_photons = V(photons_per_joule) * V(np.asarray(lf2, dtype=np.float64))
    smu = ssum([col[t] * mu_specie[t] * amu for t in range(S)])
    scs = ssum([col[t] * cross_sections[t] for t in range(S)])
    mols = m / smu
    frac = []
    for t in range(3):
        wi = col[t] * cross_sections[t] / scs
        ad = wi * frac_dest[t] * n_photons
        at = col[t] * mols
        x0 = (ad / at).nan_to_num()
        fr = (0.99 - (-x0).exp() * 0.99).nan_to_num()
        with np.errstate(all="ignore"):
            q = (at / amu).f64()
        fr = V(0.0).where(q < 1e-10, fr)
        fr = V(0.99).where(q < 0, fr)
        frac.append(fr)
    p = [col[t] * frac[t] for t in range(3)]
    new = list(col)
    new[2] = col[2] + p[0] * 2.0
    new[3] = col[3] + p[2]
    new[4] = col[4] + p[1]
    new[5] = col[5] + (p[2] + p[1])
    new[0] = col[0] - p[0]
    new[1] = col[1] - p[1]
    new[2] = new[2] - p[2]
    rows_v = np.array(f, dtype=LD)
    rows_e = np.zeros(f.shape)
    for t in range(S):
        rows_v[ns, t] = new[t].v
        rows_e[ns, t] = new[t].e
    allc = [V(rows_v[:, t], rows_e[:, t]) for t in range(S)]
    tot = ssum(allc)
    out_v, out_e = np.empty((n, S)), np.empty((n, S))
    for t in range(S):
        q = allc[t] / tot
        out_v[:, t], out_e[:, t] = q.f64(), q.e
    return dict(f_un_new=out_v, f_un_new_bound=out_e, frac_destroyed=np.stack([x.f64() for x in frac], axis=1),
                frac_destroyed_bound=np.stack([x.e for x in frac], axis=1))


def tables(f, mu_specie, gamma, cross_sections):
    col = _cols(np.asarray(f, dtype=np.float64))
    S = len(col)
    sf = ssum(col)
    return tuple(ssum([col[t] * tab[t] for t in range(S)]) / sf for tab in (mu_specie, gamma, cross_sections))


def _coeff(q):
    x = q.nan_to_num()
    with np.errstate(all="ignore"):
        pos = x.v >= 0
    return (x + 1.0).where(pos, x.exp())


def _clamps(E, T, mass, mu, gam, c):
    gmk = gam * mass * c["k"]
    mm = mu * c["m_h"]
    lo, hi = V(c["t_cmb"]) * gmk / mm, V(c["t_max"]) * gmk / mm
    E, e_lo = clamp_low(E, lo)
    E, e_hi = clamp_high(E, hi)
    T, t_lo = clamp_low(T, V(np.full(T.v.shape, c["t_cmb"])))
    T, t_hi = clamp_high(T, V(np.full(T.v.shape, c["t_max"])), strict=False)
    return E, T, dict(zip(COUNTS, (e_lo, e_hi, t_lo, t_hi)))


def _spread(pt, arr, width=None):
    """An array over the particles with ptypes != 1 onto all particles (0 elsewhere)."""
    out = np.zeros(pt.shape if width is None else pt.shape + (width,))
    out[pt != 1] = np.asarray(arr, dtype=np.float64)
    return out


def _finish(out, E_in, E, counts):
    with np.errstate(all="ignore"):
        out["totals"] = dict(E_before=float(np.sum(E_in.astype(LD))), E_after=float(np.sum(E.v)))
        out["totals_bound"] = dict(E_before=TAU * float(np.sum(np.abs(np.nan_to_num(E_in)))),
                                   E_after=float(np.sum(np.nan_to_num(E.e, posinf=DMAX))) + TAU * float(np.sum(np.nan_to_num(_f(E.v)))))
    out["counts"] = counts
    return out


def _pack(names, vals):
    out = {}
    for nm, v in zip(names, vals):
        out[nm], out[nm + "_bound"] = v.f64(), v.e
    return out


def heat_bookkeeping(f_un, ptypes, masses, mu_before, E_internal, T, lf2, mu_specie, gamma, cross_sections, t_cmb, t_max, k, m_h):
    pt = np.asarray(ptypes, dtype=np.float64)
    E_in, T_in = np.asarray(E_internal, dtype=np.float64), np.asarray(T, dtype=np.float64)
    mass = V(np.asarray(masses, dtype=np.float64))
    mu, gam, cross = tables(f_un, mu_specie, gamma, cross_sections)
    gas = pt == 0
    E0 = V(E_in)
    c0 = _coeff(V(_spread(pt, lf2)) / E0)
    E1 = E0 * c0
    n_part = mass / (V(m_h) * V(np.asarray(mu_before, dtype=np.float64)))
    T1 = E1 / (n_part * gam * k)
    E, Tn = E1.where(gas, E0), T1.where(gas, V(T_in))
    E, Tn, counts = _clamps(E, Tn, mass, mu, gam, dict(t_cmb=t_cmb, t_max=t_max, k=k, m_h=m_h))
    out = _pack(("mu_array", "gamma_array", "cross_array", "E_internal", "T"), (mu, gam, cross, E, Tn))
    return _finish(out, E_in, E, counts)


def cool_bookkeeping(final_comp, energy, ptypes, masses, sizes, E_internal, T, velocities, lf2, momentum, mu_specie, gamma,
                     cross_sections, dt, t_cmb, t_max, cooling_timescale, sb, k, m_h):
    pt = np.asarray(ptypes, dtype=np.float64)
    E_in, T_in = np.asarray(E_internal, dtype=np.float64), np.asarray(T, dtype=np.float64)
    mass, h = V(np.asarray(masses, dtype=np.float64)), V(np.asarray(sizes, dtype=np.float64))
    mu, gam, cross = tables(final_comp, mu_specie, gamma, cross_sections)
    gas, dust = pt == 0, pt == 2
    E0, T0 = V(E_in), V(T_in)
    n_part = mass / (V(m_h) * mu)
    c1 = _coeff(-(V(np.asarray(energy, dtype=np.float64)) * n_part) / E0)
    c1 = c1 * (V(-dt / cooling_timescale) * (T0 / 1e4).root(2, EPS)).exp()
    Eg = E0 * c1
    Tg = Eg / (n_part * gam * k)
    h2 = h * h
    optd = 1.0 - (-(n_part * cross) * (9.0 / (V(4 * np.pi) * h2))).exp()
    den = optd * 4.0 * np.pi * h2 * sb * 1e-5 * dt
    Td = (V(_spread(pt, lf2)) / den + V(t_cmb).root(6, TRANS)).root(6, TRANS)
    Ed = n_part * k * Td * gam
    E = Eg.where(gas, Ed.where(dust, E0))
    Tn = Tg.where(gas, Td.where(dust, T0))
    E, Tn, counts = _clamps(E, Tn, mass, mu, gam, dict(t_cmb=t_cmb, t_max=t_max, k=k, m_h=m_h))
    vel = V(np.asarray(velocities, dtype=np.float64)) + V(_spread(pt, momentum, 3))
    vel = vel.where((pt != 1)[:, None], V(np.asarray(velocities, dtype=np.float64)))
    out = _pack(("mu_array", "gamma_array", "cross_array", "E_internal", "T", "velocities"), (mu, gam, cross, E, Tn, vel))
    return _finish(out, E_in, E, counts)


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the elements that are not equal (NaN with NaN counts as equal)."""
    got, ref, bound = np.asarray(got), np.asarray(ref), np.asarray(bound)
    with np.errstate(all="ignore"):
        same = (got == ref) | (np.isnan(got) & np.isnan(ref))
        r = np.where(same, 0.0, np.abs(got - ref) / bound)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


def assert_within(name, got, ref, bound, who=""):
    w = worst_ratio(got, ref, bound)
    assert w <= 1.0, "%s %s: |difference| is %.3g of the bound at the worst element" % (who, name, w)
    return w
