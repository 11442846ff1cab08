"""NumPy restatement of the reference's rad_cooling (nsc:1019-1176) - the yardstick of the cool_* tests.  Written from
the formulas (include/sphx.h, sphx_rad_cooling), not from the reference's text; vectorised over (N, K).

Per pair (row j, p = neighbor[j,k]) everything depends on p's own data and r^2 = |x_p - x_j|^2 (`pair_terms`, the
mirror of sphx_cool_pair.h); the rows' seven sums and six scalars follow; the scatter is performed with np.add.at on the
row-major flattened list, i.e. every particle adds the rows that hold it in ascending row index - the order of the
reference's loop and of the library's transposed gather.  Then the elementwise epilogue.  The two np.min calls of
nsc:1089, 1094 are read as np.minimum.  An entry outside [0, N) contributes nothing; the
coefficients of a neighbour whose T is not in (0, inf) are zero.

Error bounds: every output comes with a first-order "<name>_bound", derived, not tuned.
  EPS = 2^-52.  TAU = 1e-12 sum|term| for every sum that may be evaluated in another order: the seven row
  sums (NumPy adds a selected row pairwise, the library in list order).  ULPS = 16 EPS stands for the handful of correctly
  rounded operations around each product or quotient (rad_oracle.ULPS).  COEF = 16 EPS relative on each of the five
  temperature coefficients: at most six correctly rounded operations plus two of pow / log / sqrt; the HIP programming
  guide's table of device math functions gives pow and log within 2 ulp and sqrt within 1 in double precision (1 for
  the host libm) - no copy of that table is installed beside the toolchain this was written with, so the figure is
  quoted from the public document, not re-read.
  Weigh2 = c q^3 / (64 pi d^9) with q = h(m)^2 - r^2 cancels near the edge of the support: h(m)^2 carries a pow
  (4 EPS), r^2 three squares and two additions of differences (4 EPS of r^2 as a sum of non-negative terms, the
  differences themselves being exact to EPS each), so dq = 4 EPS (h^2 + r^2) and dW = 3 |c| q^2 dq / (64 pi d^9) +
  ULPS |W| - an ABSOLUTE bound, valid through q = 0, where the masks [W > 0] may fall either way and every masked term
  is itself O(q^3): the masks introduce no discontinuity.
  These propagate linearly: through the row sums (d sum = sum d term + TAU sum|term|), the quotients of the row scalars
  (relative errors add), the caps at 0.9999 (1-Lipschitz; a value further above the cap than its bound has bound 0), the
  gather (d = sum (d scalar rel_w + scalar d rel_w) + TAU sum|term|), the division by rel + 1e-90, and the epilogue's
  sums and differences (absolute errors add).  mult_factor = 0.9999 / mf2 above the cap and 1 below is continuous
  at the cap with slope <= 1/0.9999, so within its bound of the cap d mult = d mf2 / 0.9999; exactly AT the cap
  (quirk 2) it jumps by 1e-4 - the fixtures hold no such particle (asserted where they are made).
"""
import numpy as np

EPS = 2.0 ** -52
TAU = 1e-12
ULPS = 16 * EPS
COEF = 16 * EPS
CAP = 0.9999
K_B = 1.380649e-23
AMU = 1.66053906892e-27
M_H = 1.0008 * AMU
M_0 = 10 ** 1.5 * 1.989e30
OUTPUTS = ("final_comp", "energy", "rec_array", "row_table")


def _fin(a):
    return np.where(np.isfinite(a), a, 0.0)


def _pos(v):
    """x [x > 0] of nan_to_num(x)."""
    return np.where(v > 0.0, np.minimum(v, np.finfo(np.float64).max), 0.0)


def coefficients(T, gas, k=K_B):
    """-> (5, N): H_eff, He_eff, H2_eff, e_H, e_He; zero for non-gas and for T not in (0, inf)."""
    T = np.asarray(T, dtype=np.float64)
    ok = gas & (T > 0.0) & np.isfinite(T)
    Ts = np.where(ok, T, 1.0)
    t4 = Ts / 10000.0
    lt = np.log(t4)
    c = np.array([4.13e-19 * t4 ** (-0.7131 - 0.0115 * lt), 2.72e-19 * t4 ** (-0.789), 7.3e-23 * 0.5 * (Ts / 100.0) ** 0.5,
                  (0.684 - 0.0416 * lt + 0.54 * t4 ** 0.37) * k * Ts, (0.684 - 0.0416 * np.log(t4 / 4.0)) * k * Ts])
    return np.where(ok[None, :], c, 0.0)


def pair_terms(x, m, gas, mu, f, nb, d, m_0=M_0, m_h=M_H):
    """The per-neighbour term -> dict of (N, K) arrays: p (the neighbour, 0 where the entry is invalid), valid, relw,
    ne, nHp, nHep, nH0, and the absolute bounds relw_b, n_b (of base = W / (mu m_h), to be multiplied by f)."""
    n = x.shape[0]
    valid = (nb >= 0) & (nb < n)
    p = np.where(valid, nb, 0)
    h2 = (m / m_0) ** (2.0 / 3.0) * d ** 2
    c = m * 315 * (m_0 / m) ** 3
    den = 64 * np.pi * d ** 9
    winv = 1.0 / (c * h2 ** 3 / den)
    r2 = np.sum((x[p] - x[:, None, :]) ** 2, axis=2)
    q = h2[p] - r2
    on = valid & gas[p]
    W = np.where(on, c[p] * q ** 3 / den, 0.0)
    dq = 4 * EPS * (h2[p] + r2)
    W_b = np.where(on, 3 * np.abs(c[p]) * q ** 2 * dq / den + ULPS * np.abs(W), 0.0)
    mm = mu[p] * m_h
    base = W / mm
    out = dict(p=p, valid=valid, relw=np.where(W > 0.0, _pos(W) * winv[p], 0.0), relw_b=W_b * winv[p] + ULPS * np.abs(W) * winv[p],
               base_b=W_b / np.abs(mm) + ULPS * np.abs(base))
    for nm, col in (("ne", 5), ("nHp", 3), ("nHep", 4), ("nH0", 2)):
        out[nm] = _pos(base * f[p, col])
        out[nm + "_b"] = out["base_b"] * np.abs(f[p, col]) + ULPS * out[nm]
    return out


def _sum(term, term_b):
    """Row sums over K of non-negative terms and their bounds."""
    s = np.sum(term, axis=1)
    return s, np.sum(term_b, axis=1) + TAU * s


def _cap(v, b):
    """np.minimum(v, CAP) and its bound."""
    with np.errstate(invalid="ignore"):
        return np.minimum(v, CAP), np.where(v - b > CAP, 0.0, b)


def cooling(positions, particle_type, masses, f_un, neighbor, mu_array, T, dt, d, m_0=M_0, m_h=M_H, k=K_B):
    """-> dict: final_comp (N,S), energy (N,), rec_array (S,N), row_table (N,6) [f_Hn, f_H, f_He, f_e, E_H, E_He; the f's
    through nan_to_num], row_contributes (N,), row_num_e (N,), mf2 (N,), "<name>_bound" for the four outputs."""
    x = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    n = x.shape[0]
    pt = np.asarray(particle_type, dtype=np.float64)
    m = np.asarray(masses, dtype=np.float64)
    mu = np.asarray(mu_array, dtype=np.float64)
    f = np.nan_to_num(np.asarray(f_un, dtype=np.float64))
    S = f.shape[1]
    nb = np.asarray(neighbor, dtype=np.int64)
    gas = pt == 0
    with np.errstate(all="ignore"):
        pr = pair_terms(x, m, gas, mu, f, nb, float(d), m_0, m_h)
        p = pr["p"]
        co = coefficients(T, gas, k)
        Hf, Hef, H2f, eH, eHe = (c[p] for c in co)
        contributes = gas & np.any(pr["valid"] & gas[p], axis=1)
        rowm = contributes[:, None]
        ne, ne_b = np.where(rowm, pr["ne"], 0.0), np.where(rowm, pr["ne_b"], 0.0)
        nH0, nH0_b = np.where(rowm, pr["nH0"], 0.0), np.where(rowm, pr["nH0_b"], 0.0)
        num_e, num_e_b = _sum(ne, ne_b)
        A, A_b = _sum(Hf * ne, Hf * ne_b + COEF * Hf * ne)
        B, B_b = _sum(Hef * ne, Hef * ne_b + COEF * Hef * ne)
        SH, SH_b = _sum(Hf * ne * eH, Hf * eH * ne_b + 2 * COEF * Hf * ne * eH)
        SHe, SHe_b = _sum(Hef * ne * eHe, Hef * eHe * ne_b + 2 * COEF * Hef * ne * eHe)
        nHp, nHp_b = _sum(np.where(rowm, pr["nHp"], 0.0), np.where(rowm, pr["nHp_b"], 0.0))
        nHep, nHep_b = _sum(np.where(rowm, pr["nHep"], 0.0), np.where(rowm, pr["nHep_b"], 0.0))
        Cn, Cn_b = _sum(H2f * nH0, H2f * nH0_b + COEF * H2f * nH0)
        # row scalars
        top = A * nHp + B * nHep
        fe_raw = top / num_e * dt
        fe_rel = (A_b * nHp + A * nHp_b + B_b * nHep + B * nHep_b) / top + num_e_b / num_e + ULPS
        fe, fe_b = _cap(fe_raw, np.abs(fe_raw) * fe_rel)
        sH, sHe = np.nan_to_num(A / (A + B)), np.nan_to_num(B / (A + B))
        s_rel = (A_b + B_b) / (A + B) + ULPS
        sH_b, sHe_b = sH * (A_b / A + s_rel), sHe * (B_b / B + s_rel)
        fH, fHe = fe * sH, fe * sHe
        fH_b = fe_b * sH + fe * sH_b + ULPS * np.abs(fH)
        fHe_b = fe_b * sHe + fe * sHe_b + ULPS * np.abs(fHe)
        fHn, fHn_b = _cap(Cn * dt, Cn_b * dt + ULPS * Cn * dt)
        EH, EHe = SH * sH * dt, SHe * sHe * dt
        EH_b = (SH_b * sH + SH * sH_b) * dt + ULPS * np.abs(EH)
        EHe_b = (SHe_b * sHe + SHe * sHe_b) * dt + ULPS * np.abs(EHe)
        table = np.stack([np.nan_to_num(fHn), np.nan_to_num(fH), np.nan_to_num(fHe), np.nan_to_num(fe), EH, EHe], axis=1)
        table_b = _fin(np.stack([fHn_b, fH_b, fHe_b, fe_b, EH_b, EHe_b], axis=1))
        table = np.where(rowm, table, 0.0)
        table_b = np.where(rowm & ~np.isnan(table_b), table_b, 0.0)
        # ---- the scatter, in ascending row order ----
        w, w_b = np.where(rowm, pr["relw"], 0.0), np.where(rowm, pr["relw_b"], 0.0)
        me, mh = pr["ne"] > 0.0, pr["nH0"] > 0.0
        # a mask that falls the other way changes a term by at most (scalar + its bound) (rel_w + its bound) with
        # rel_w <= its bound there, which the products below cover: the mask is applied to the VALUE only
        flat_p = p.ravel()
        acc = np.zeros((7, n)); acc_b = np.zeros((7, n))
        spec = ((4, None), (5, None), (0, mh), (1, me), (2, me), (3, me))
        for slot, (col, mask) in enumerate(spec):
            sc, sc_b = table[:, col][:, None], table_b[:, col][:, None]
            val = np.nan_to_num(sc * w) if mask is None else sc * np.where(mask, w, 0.0)
            b = sc_b * (w + w_b) + np.abs(sc) * w_b
            np.add.at(acc[slot], flat_p, val.ravel())
            np.add.at(acc_b[slot], flat_p, (b + TAU * np.abs(val)).ravel())
        np.add.at(acc[6], flat_p, w.ravel())
        np.add.at(acc_b[6], flat_p, (w_b + TAU * w).ravel())
        rel, rel_b = acc[6], acc_b[6]
        den = rel + 1e-90

        def quot(a, a_b):
            v = a / den
            return v, a_b / den + np.abs(v) * rel_b / den + ULPS * np.abs(v)
        e3, e3_b = quot(acc[0], acc_b[0])
        e4, e4_b = quot(acc[1], acc_b[1])
        r2, r2_b = quot(acc[2], acc_b[2])
        r3, r3_b = quot(acc[3], acc_b[3])
        r4, r4_b = quot(acc[4], acc_b[4])
        r5, r5_b = quot(acc[5], acc_b[5])
        r2, r3, r4, r5 = (np.nan_to_num(v) for v in (r2, r3, r4, r5))
        # ---- epilogue ----
        f0, f1, f2, f3, f4, f5 = (f[:, c].copy() for c in range(6))
        Hp, Hep, el = f5 * r3, f5 * r4, f5 * r5
        Hp_b, Hep_b, el_b = (f5 * b + ULPS * np.abs(v) for v, b in ((Hp, r3_b), (Hep, r4_b), (el, r5_b)))
        qa, qb = np.nan_to_num(Hp / f3), np.nan_to_num(Hep / f4)
        qa_b, qb_b = _fin(Hp_b / np.abs(f3)) + ULPS * np.abs(qa), _fin(Hep_b / np.abs(f4)) + ULPS * np.abs(qb)
        mf2 = np.maximum(qa, qb)
        mf2_b = np.maximum(qa_b, qb_b)
        mult = mf2.copy()
        mult[mf2 > CAP] = CAP / mf2[mf2 > CAP]
        mult[mf2 < CAP] = 1.0
        mult[f5 < 1e-10] = 0.0
        mult_b = np.where((mf2 + mf2_b >= CAP) & ~(f5 < 1e-10), mf2_b / CAP + ULPS, 0.0)
        energy = e3 * f3 + e4 * f4
        energy_b = e3_b * np.abs(f3) + e4_b * np.abs(f4) + ULPS * (np.abs(e3 * f3) + np.abs(e4 * f4))

        def moved(v, v_b):
            t = v * mult
            return t, v_b * mult + np.abs(v) * mult_b + ULPS * np.abs(t)
        tH, tH_b = moved(Hp, Hp_b)
        tHe, tHe_b = moved(Hep, Hep_b)
        te, te_b = moved(el, el_b)
        g1, g1_b = f1 + tHe, tHe_b + ULPS * (np.abs(f1) + np.abs(tHe))
        g2, g2_b = f2 + tH, tH_b + ULPS * (np.abs(f2) + np.abs(tH))
        g3, g3_b = f3 - tH, tH_b + ULPS * (np.abs(f3) + np.abs(tH))
        g4, g4_b = f4 - tHe, tHe_b + ULPS * (np.abs(f4) + np.abs(tHe))
        g5, g5_b = f5 - te, te_b + ULPS * (np.abs(f5) + np.abs(te))
        r2c, r2c_b = _cap(r2, r2_b)
        H2 = g2 * r2c
        H2_b = g2_b * r2c + np.abs(g2) * r2c_b + ULPS * np.abs(H2)
        g0, g0_b = f0 + H2 / 2.0, H2_b / 2.0 + ULPS * (np.abs(f0) + np.abs(H2))
        g2, g2_b = g2 - H2, g2_b + H2_b + ULPS * (np.abs(g2) + np.abs(H2))
        comp = f.T.copy()
        comp_b = np.zeros_like(comp)
        for c, (v, b) in enumerate(((g0, g0_b), (g1, g1_b), (g2, g2_b), (g3, g3_b), (g4, g4_b), (g5, g5_b))):
            comp[c], comp_b[c] = v, b
        tot = np.sum(comp, axis=0)
        tot_b = np.sum(comp_b, axis=0) + ULPS * np.sum(np.abs(comp), axis=0)
        final = comp / tot
        final_b = comp_b / np.abs(tot) + np.abs(final) * tot_b / np.abs(tot) + ULPS * np.abs(final)
        rec = np.zeros((S, n)); rec_b = np.zeros((S, n))
        rec[2], rec[3], rec[4], rec[5] = r2c, r3, r4, r5
        rec_b[2], rec_b[3], rec_b[4], rec_b[5] = r2c_b, r3_b, r4_b, r5_b
    return dict(final_comp=final.T.copy(), energy=energy, rec_array=rec, row_table=table,
                final_comp_bound=_fin(final_b).T.copy(), energy_bound=_fin(energy_b), rec_array_bound=_fin(rec_b),
                row_table_bound=table_b, row_contributes=contributes, row_num_e=np.where(contributes, num_e, -1.0), mf2=mf2)


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
