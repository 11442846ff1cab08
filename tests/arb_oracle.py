"""NumPy restatement of the reference's arbitrary-point samplers (nsc:1422-1527) - the yardstick of the *_arb tests.

Written from the formulas, not from the reference's text.  With C = 315/(64 pi), h(m) = (m/m_0)^(1/3) d,
g = [type == 0], u = [type == 2], r^2 = |x_k - x_0|^2 over the members k of a point's ball:

    Wg = m C h^-9 (h^2 - r^2)^3          Wd = m C s^-9 (s^2 - r^2)^3,  s = sizes          (unclipped)
    density          sum of the positive Wg g
    dust_density     sum of the positive Wd u
    temperature      nan_to_num(sum a / sum b) over a = Wg g T > 0, b = Wg g
    dust_temperature nan_to_num(sum Wd u T / sum Wd u) over Wd u > 0
    photoionization  sum w nan_to_num(value) / sum w over w = (1 - r^2/h^2)^3 g n_part > 0        (0/0 stays NaN)
    every function returns 0 for a ball of at most one member.

Error bounds (derived, not tuned).  A sum of c non-negative terms W_k = f_k (1 - q_k^2)^3, f = m C / h^3, each
evaluated from q^2 = r^2/h^2 carrying a few ulp: d(1 - q^2)^3 = 3 (1 - q^2)^2 d(q^2), so two correct evaluations differ
by at most (c + 32) 2^-52 S with S = sum f_k (1 - q_k^2)^2 over the positive terms (c ulp of summation, 32 ulp of
per-term evaluation, the lower power absorbing the cancellation at the edge of the support).  A quotient num/den
inherits (b_num + |ref| b_den) / den.  A term within 8 ulp of the mask's edge may fall on either side of "> 0"; it is
then smaller than the bound it would add to, so no point needs to be excluded.
"""
import numpy as np

C_W6 = 315.0 / (64.0 * np.pi)
EPS = 2.0 ** -52
FIELDS = ("density", "dust_density", "temperature", "dust_temperature", "photoionization")


def to_csr(rows):
    """sequence of index sequences -> (row_start (M+1) int64, members int64)."""
    lens = np.fromiter((len(r) for r in rows), dtype=np.int64, count=len(rows))
    row_start = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(lens, out=row_start[1:])
    members = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows]) if row_start[-1] else np.zeros(0, np.int64)
    return row_start, members


def brute_ball(points, arb_points, radius, chunk=256):
    """The exact (eps = 0) ball by brute force -> CSR; members ascending within a row."""
    pts = np.asarray(points, dtype=np.float64)
    q = np.asarray(arb_points, dtype=np.float64)
    R2 = float(radius) * float(radius)
    rows = []
    with np.errstate(invalid="ignore"):
        for s in range(0, q.shape[0], chunk):
            dx = pts[None, :, 0] - q[s:s + chunk, None, 0]
            dy = pts[None, :, 1] - q[s:s + chunk, None, 1]
            dz = pts[None, :, 2] - q[s:s + chunk, None, 2]
            inside = dx * dx + dy * dy + dz * dz <= R2
            rows.extend(np.nonzero(row)[0] for row in inside)
    return to_csr(rows)


def _row_sum(row_id, values, mask, m):
    return np.bincount(row_id[mask], weights=values[mask], minlength=m) if mask.any() else np.zeros(m)


def fields(points, mass, particle_type, sizes, T, n_part, value, d, m_0, arb_points, row_start, members):
    """-> dict: the five outputs (M,), "count" (row lengths), and per output "<name>_bound" (M,): the largest
    |x - ref| two correct evaluations may differ by (module docstring).  sizes / T / n_part / value may be None: the
    outputs that need them are left out.  Rows are summed in list order (np.bincount adds in input order)."""
    pts = np.asarray(points, dtype=np.float64)
    q = np.asarray(arb_points, dtype=np.float64).reshape(-1, 3)
    m = q.shape[0]
    row_start = np.asarray(row_start, dtype=np.int64)
    members = np.asarray(members, dtype=np.int64)
    lens = np.diff(row_start)
    row_id = np.repeat(np.arange(m), lens)
    k = members
    gate = lens > 1
    ms = np.asarray(mass, dtype=np.float64)[k]
    t = np.asarray(particle_type, dtype=np.float64)[k]
    g = (t == 0).astype(np.float64)
    u = (t == 2).astype(np.float64)
    out = {"count": lens.copy()}
    with np.errstate(all="ignore"):
        diff = pts[k] - q[row_id]
        r2 = np.sum(diff ** 2, axis=1)
        h = np.cbrt(ms / m_0) * d
        h2 = h * h
        fg = ms * C_W6 / (h2 * h)
        tg = 1.0 - r2 / h2
        Wg = fg * tg ** 3 * g
        Sg_t = fg * tg ** 2 * g                           # the bound's per-term scale
        pos = Wg > 0
        cnt = np.bincount(row_id[pos], minlength=m)
        dens = _row_sum(row_id, Wg, pos, m)
        out["density"] = np.where(gate, dens, 0.0)
        out["density_bound"] = (cnt + 32) * EPS * _row_sum(row_id, Sg_t, pos, m)

        def quotient(num_terms, den_terms, num_scale, den_scale, mask, nan_to_num):
            c = np.bincount(row_id[mask], minlength=m)
            num, den = _row_sum(row_id, num_terms, mask, m), _row_sum(row_id, den_terms, mask, m)
            b_num = (c + 32) * EPS * _row_sum(row_id, np.abs(num_scale), mask, m)
            b_den = (c + 32) * EPS * _row_sum(row_id, np.abs(den_scale), mask, m)
            ref = num / den
            if nan_to_num:
                ref = np.nan_to_num(ref)
            bound = (b_num + np.abs(ref) * b_den) / np.abs(den)
            bound = np.where(np.isfinite(bound), bound, 0.0)
            return np.where(gate, ref, 0.0), bound

        if T is not None:
            Tk = np.asarray(T, dtype=np.float64)[k]
            a = Wg * Tk
            out["temperature"], out["temperature_bound"] = quotient(a, Wg, Sg_t * Tk, Sg_t, a > 0, True)
        if sizes is not None:
            s = np.asarray(sizes, dtype=np.float64)[k]
            s2 = s * s
            fd = ms * C_W6 / (s2 * s)
            td = 1.0 - r2 / s2
            Wd = fd * td ** 3 * u
            Sd_t = fd * td ** 2 * u
            posd = Wd > 0
            cd = np.bincount(row_id[posd], minlength=m)
            out["dust_density"] = np.where(gate, _row_sum(row_id, Wd, posd, m), 0.0)
            out["dust_density_bound"] = (cd + 32) * EPS * _row_sum(row_id, Sd_t, posd, m)
            if T is not None:
                out["dust_temperature"], out["dust_temperature_bound"] = quotient(Wd * Tk, Wd, Sd_t * Tk, Sd_t, posd, True)
        if n_part is not None and value is not None:
            npk = np.asarray(n_part, dtype=np.float64)[k]
            vk = np.nan_to_num(np.asarray(value, dtype=np.float64)[k])
            w = tg ** 3 * g * npk
            ws = tg ** 2 * g * npk
            out["photoionization"], out["photoionization_bound"] = quotient(w * vk, w, ws * vk, ws, w > 0, False)
    for name in FIELDS:                                   # a gate zero is an exact zero
        if name + "_bound" in out:
            out[name + "_bound"] = np.where(gate, out[name + "_bound"], 0.0)
    return out


def assert_within(name, x, ref, bound, what=""):
    """|x - ref| <= bound elementwise; NaN must match NaN; where ref is an exact gate zero so must x be."""
    x, ref, bound = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert x.shape == ref.shape, (what, name, x.shape, ref.shape)
    nan_x, nan_r = np.isnan(x), np.isnan(ref)
    assert np.array_equal(nan_x, nan_r), "%s %s: NaN pattern differs at %s" % (what, name, np.nonzero(nan_x != nan_r)[0][:8])
    ok = nan_r | (x == ref)
    with np.errstate(invalid="ignore"):
        ok |= np.abs(x - ref) <= bound
    if not ok.all():
        bad = np.nonzero(~ok)[0]
        worst = bad[np.argmax(np.abs(x - ref)[bad] / np.maximum(bound[bad], 1e-300))]
        raise AssertionError("%s %s: %d of %d points beyond the bound; worst at %d: got %r, ref %r, |diff| %.3e, bound %.3e"
                             % (what, name, bad.size, x.size, worst, x[worst], ref[worst], abs(x[worst] - ref[worst]),
                                bound[worst]))
