"""NumPy restatement of the gravitational potential of include/sphx.h (sphx_gravity_direct_pot):

    phi_i = -G sum_{j != i} m_j / sqrt(|x_j - x_i|^2 + eps^2)          [J/kg]

Row i is left out of its own sum BY INDEX (np.where picks +0.0 for it: nothing is added and taken off again); a different
row at the same position contributes -G m_j / eps, and with eps = 0 and r = 0 nothing - as a coincident pair does in
oracle.gravity_direct.  Chunked like that function, and like it returns sum_j |term_ij| beside the sum: the scale a row's
round-off is measured against.  U = 1/2 sum_i m_i phi_i.

Nothing here is tuned to the library's output: every line follows the header's definition."""
import numpy as np

G_NEWTON = 6.67430e-11


def potential_at(targets, points, mass, softening, G=G_NEWTON, exclude=None, chunk=512):
    """phi at targets (t,3) of the sources (points, mass) -> (phi (t,), sum_j |term_tj| (t,)).  exclude (t,), optional:
    the index of the source each target leaves out (a negative entry: none)."""
    xt = np.asarray(targets, dtype=np.float64)
    p = np.asarray(points, dtype=np.float64)
    m = np.asarray(mass, dtype=np.float64)
    e2 = float(softening) ** 2
    out = np.zeros(len(xt))
    out_abs = np.zeros(len(xt))
    cols = np.arange(len(p))
    for a in range(0, len(xt), chunk):
        d = p[None, :, :] - xt[a:a + chunk, None, :]                  # (c, n, 3)
        r2 = np.sum(d * d, axis=2) + e2
        with np.errstate(all="ignore"):
            t = np.where(r2 > 0, m[None, :] / np.sqrt(r2), 0.0)
        if exclude is not None:
            t = np.where(cols[None, :] == np.asarray(exclude)[a:a + chunk, None], 0.0, t)
        out[a:a + chunk] = -G * np.sum(t, axis=1)
        out_abs[a:a + chunk] = G * np.sum(np.abs(t), axis=1)
    return out, out_abs


def potential_direct(points, mass, softening, G=G_NEWTON, chunk=512):
    """phi_i of every row of the cloud, self left out by index -> (phi (n,), sum_j |term_ij| (n,))."""
    n = len(np.asarray(points))
    return potential_at(points, points, mass, softening, G, exclude=np.arange(n), chunk=chunk)


def total(mass, phi):
    """U = 1/2 sum m phi, as a plain NumPy sum (the library's ordered total: tests/census_oracle.ordered_totals)."""
    return 0.5 * float(np.sum(np.asarray(mass, dtype=np.float64) * np.asarray(phi, dtype=np.float64)))
