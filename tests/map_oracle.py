"""NumPy restatement of the projected maps (include/sphx.h sphx_project_maps) - the yardstick of the map tests.

Written from the definitions.  The image: axes = (a_u, a_v), centre (c_u, c_v), half-widths (w_u, w_v), n_u x n_v pixels,
pixel (i, j) centred at u_i = c_u - w_u + (i + 1/2) 2 w_u / n_u (left to right), v_j likewise; arrays are (n_v, n_u).
Particle k: R = cbrt(m/m_0) d for gas (type 0), sizes for dust (type 2), none for any other type; with
s = R^2 - ((u_i - x_u)^2 + (v_j - x_v)^2) its term at a pixel is c s^3 sqrt(s) for s > 0, c = m (9 / (2 pi)) / R^9.  A gas or
dust row with a non-finite coordinate, mass or radius, or R <= 0, is skipped; with depth = (lo, hi) only rows with
lo <= x_w < hi count.

    gas_column        sum of the gas terms            dust_column       sum of the dust terms
    gas_temperature   sum(t T) / sum(t) over the gas terms with t T > 0; 0 where the denominator is 0
    dust_temperature  sum(t T) / sum(t) over the dust terms with t > 0; 0 where the denominator is 0
    count             the rows with s > 0 at the pixel

Every pixel's sums take their terms in ascending particle index (the loop below runs over the particles; NumPy adds a
particle's term to every pixel at once).  Each operation is rounded on its own, in the order of
sph-code_amd/csrc/sphx_map_pair.h; what may differ from the library by an ulp is cbrt alone.

Beside the fields: "<field>_abs" - the sum of |term| per pixel (gas_temperature_abs / dust_temperature_abs: of the
numerator's terms; "*_den_abs" of the denominator's) -, "edge" - the (particle, pixel) pairs with |s| <= 8 2^-52 R^2, where
an ulp of R decides whether the pair counts -, "box_edge" - the (particle, pixel column or row) pairs whose centre lies
within 8 2^-52 R of the bounding box's side, where an ulp decides whether a tile is listed -, "skipped", and "pairs": the
(particle, 16 x 16 tile) pairs, a particle being listed in the tiles that hold a pixel with |u_i - x_u| <= R and
|v_j - x_v| <= R."""
import numpy as np

C_MAP = 9.0 / (2.0 * np.pi)
TILE = 16
EPS = 2.0 ** -52
FIELDS = ("gas_column", "dust_column", "gas_temperature", "dust_temperature", "count")


def centres(c, w, n):
    """u_i = c - w + (i + 1/2) 2 w / n for i = 0 .. n - 1, evaluated left to right."""
    i = np.arange(int(n), dtype=np.float64)
    return np.float64(c) - np.float64(w) + (i + 0.5) * 2.0 * np.float64(w) / np.float64(int(n))


def term(c, s):
    """c s^3 sqrt(s), in the library's order."""
    return c * (s * s * s * np.sqrt(s))


def coeff(m, R):
    r2 = R * R
    r4 = r2 * r2
    return m * C_MAP / (r4 * r4 * R)


def radius(ptype, m, size, d, m_0):
    """R of a row, or None for a type without a footprint."""
    if ptype == 0.0:
        return np.cbrt(m / m_0) * d
    if ptype == 2.0:
        return np.float64(size)
    return None


def project(points, mass, particle_type, sizes, T, d, m_0, axes=(1, 2), center=(0., 0.), half_width=(1., 1.), npix=(16, 16),
            depth=None):
    pts = np.asarray(points, dtype=np.float64)
    m_, pt_, sz_, T_ = (np.asarray(a, dtype=np.float64) for a in (mass, particle_type, sizes, T))
    au, av = int(axes[0]), int(axes[1])
    aw = 3 - au - av
    nu, nv = int(npix[0]), int(npix[1])
    u = centres(center[0], half_width[0], nu)
    v = centres(center[1], half_width[1], nv)
    shape = (nv, nu)
    z = lambda: np.zeros(shape)
    gc, dc, gn, gd, dn, dd = z(), z(), z(), z(), z(), z()
    a_gc, a_dc, a_gn, a_gd, a_dn, a_dd = z(), z(), z(), z(), z(), z()
    cnt = np.zeros(shape, dtype=np.int64)
    edge = box_edge = skipped = pairs = 0
    d = np.float64(d)
    with np.errstate(all="ignore"):
        for k in range(pts.shape[0]):
            R = radius(pt_[k], m_[k], sz_[k], d, np.float64(m_0))
            if R is None:
                continue
            xu, xv, xw, m = pts[k, au], pts[k, av], pts[k, aw], m_[k]
            if not (np.isfinite(xu) and np.isfinite(xv) and np.isfinite(xw) and np.isfinite(m) and np.isfinite(R) and R > 0.0):
                skipped += 1
                continue
            if depth is not None and not (xw >= depth[0] and xw < depth[1]):
                continue
            du, dv = u - xu, v - xv
            box_edge += int(np.count_nonzero(np.abs(np.abs(du) - R) <= 8 * EPS * R)) + int(np.count_nonzero(np.abs(np.abs(dv) - R) <= 8 * EPS * R))
            iu, iv = np.flatnonzero((du >= -R) & (du <= R)), np.flatnonzero((dv >= -R) & (dv <= R))
            if iu.size and iv.size:
                pairs += (iu[-1] // TILE - iu[0] // TILE + 1) * (iv[-1] // TILE - iv[0] // TILE + 1)
            R2 = R * R
            s = R2 - ((du * du)[None, :] + (dv * dv)[:, None])
            edge += int(np.count_nonzero(np.abs(s) <= 8 * EPS * R2))
            pos = s > 0.0
            if not pos.any():
                continue
            t = np.where(pos, term(coeff(m, R), np.where(pos, s, 1.0)), 0.0)
            cnt += pos
            if pt_[k] == 0.0:
                gc = np.where(pos, gc + t, gc); a_gc = np.where(pos, a_gc + np.abs(t), a_gc)
                tt = t * T_[k]
                mk = pos & (tt > 0.0)
                gn = np.where(mk, gn + tt, gn); gd = np.where(mk, gd + t, gd)
                a_gn = np.where(mk, a_gn + np.abs(tt), a_gn); a_gd = np.where(mk, a_gd + np.abs(t), a_gd)
            else:
                dc = np.where(pos, dc + t, dc); a_dc = np.where(pos, a_dc + np.abs(t), a_dc)
                mk = pos & (t > 0.0)
                tt = t * T_[k]
                dn = np.where(mk, dn + tt, dn); dd = np.where(mk, dd + t, dd)
                a_dn = np.where(mk, a_dn + np.abs(tt), a_dn); a_dd = np.where(mk, a_dd + np.abs(t), a_dd)
        ratio = lambda num, den: np.where(den == 0.0, 0.0, num / np.where(den == 0.0, 1.0, den))
        out = dict(gas_column=gc, dust_column=dc, gas_temperature=ratio(gn, gd), dust_temperature=ratio(dn, dd), count=cnt,
                   gas_column_abs=a_gc, dust_column_abs=a_dc, gas_temperature_abs=a_gn, gas_temperature_den_abs=a_gd,
                   dust_temperature_abs=a_dn, dust_temperature_den_abs=a_dd, edge=edge, box_edge=box_edge, skipped=skipped,
                   pairs=int(pairs), u=u, v=v)
    return out
