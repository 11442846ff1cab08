"""NumPy restatement of supernova_impulse (nsc:1192-1204) and the driver's loop over the stars (drv:350-352), in the
library's own orders (include/sphx.h, sphx_supernova_impulse):

  * candidates: the rows with ptypes == 0 by squared distance ascending, ties by ascending index (a stable sort), a NaN
    distance last;
  * the boundary by the left-to-right running sum of their masses: the prefix up to the first row whose running sum is
    not < mass_displaced (for positive finite masses this is the reference's mask `cumsum < M`);
  * true_mass in the order of sphx_ordered_totals over the selection in sorted order (ordered_total below).

Nothing here is tuned to the library's output: every line follows the reference's statement or the header's rule."""
import numpy as np

SOLAR_MASS = 1.989e30            # nsc:30
SUPERNOVA_ENERGY = 1e44          # nsc:35
MASS_DISPLACED = 194.28 * SOLAR_MASS     # nsc:1193
KICK_FRACTION = 0.736            # nsc:1200
TOT_CHUNK = 256
TOT_LANES = 256


def ordered_total(v):
    """The sum of v in sphx_ordered_totals' order: chunks of 256 consecutive entries left to right; lane l of 256 adds the
    chunks l, l + 256, ... in order; the lanes by a binary tree (l += l + 128, then 64, ...)."""
    v = np.asarray(v, dtype=np.float64)
    nchunk = (v.shape[0] + TOT_CHUNK - 1) // TOT_CHUNK
    part = np.zeros(nchunk)
    for c in range(nchunk):
        s = 0.0
        for x in v[c * TOT_CHUNK:(c + 1) * TOT_CHUNK]:
            s = s + float(x)
        part[c] = s
    lanes = np.zeros(TOT_LANES)
    for l in range(TOT_LANES):
        s = 0.0
        for c in range(l, nchunk, TOT_LANES):
            s = s + float(part[c])
        lanes[l] = s
    h = TOT_LANES // 2
    while h > 0:
        lanes[:h] = lanes[:h] + lanes[h:2 * h]
        h //= 2
    return float(lanes[0])


def dist2(points, ku):
    """nsc:1194 in NumPy's order over the three columns: (dx^2 + dy^2) + dz^2."""
    d = points - points[ku]
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def candidates(points, ptypes, ku):
    """The gas rows by (distance, index); NaN distances last, by index (np.argsort's stable kind puts NaN last)."""
    with np.errstate(all="ignore"):
        s = dist2(points, ku)
    order = np.argsort(s, kind="stable")
    return order[ptypes[order] == 0], s


def select(points, masses, ptypes, ku, mass_displaced=MASS_DISPLACED):
    """-> (selected ids in sorted order, s): the prefix of the candidates whose running sum stays < mass_displaced."""
    g, s = candidates(points, ptypes, ku)
    running = 0.0
    n_sel = 0
    with np.errstate(all="ignore"):
        for m in masses[g]:
            running = running + float(m)
            if not running < mass_displaced:
                break
            n_sel += 1
    return g[:n_sel], s


def supernova_impulse(points, masses, supernova_pos, ptypes, mass_displaced=MASS_DISPLACED, supernova_energy=SUPERNOVA_ENERGY):
    """-> (d_vels (n_sel,3), selected (n_sel,) int64, true_mass, vel)."""
    points = np.asarray(points, dtype=np.float64); masses = np.asarray(masses, dtype=np.float64)
    ptypes = np.asarray(ptypes, dtype=np.float64)
    ku = int(supernova_pos)
    sel, _ = select(points, masses, ptypes, ku, mass_displaced)
    true_mass = ordered_total(masses[sel])
    with np.errstate(all="ignore"):
        vel = np.sqrt(np.float64(2 * supernova_energy * KICK_FRACTION) / np.float64(true_mass))      # nsc:1200
        d = points[sel] - points[ku]
        s = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        d_vels = (d.T / np.sqrt(s) * vel).T                                                           # nsc:1201
    return np.ascontiguousarray(d_vels).reshape(-1, 3), sel.astype(np.int64), float(true_mass), float(vel)


def supernova_impulses(points, masses, supernova_pos, ptypes, velocities, mass_displaced=MASS_DISPLACED,
                       supernova_energy=SUPERNOVA_ENERGY):
    """drv:350-352 -> (velocities_new, [(d_vels, selected, true_mass, vel) per star])."""
    v = np.array(velocities, dtype=np.float64)
    out = []
    for ku in np.atleast_1d(supernova_pos):
        d_vels, sel, tm, vel = supernova_impulse(points, masses, ku, ptypes, mass_displaced, supernova_energy)
        v[sel] += d_vels                                                                              # (sel holds no index twice)
        out.append((d_vels, sel, tm, vel))
    return v, out


def counts(points, masses, ptypes, supernova_pos, mass_displaced=MASS_DISPLACED):
    """The two counts that do not depend on the route: selected rows at distance 0 over the stars."""
    zero = 0
    for ku in np.atleast_1d(supernova_pos):
        sel, s = select(np.asarray(points, dtype=np.float64), np.asarray(masses, dtype=np.float64),
                        np.asarray(ptypes, dtype=np.float64), int(ku), mass_displaced)
        zero += int(np.count_nonzero(s[sel] == 0.0))
    return {"zero_distance": zero}


def event_dt(dt_0, ct):
    """drv:358: dt = min(dt_0 / 100, ct)."""
    return min(dt_0 / 100, ct)
