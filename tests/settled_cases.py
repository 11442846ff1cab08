"""States for the tests of the sums that are NaN before they are finished (sphx_settled.h; test helper, no test of its
own): N = 1536 particles in three clumps of 512, further apart than any kNN radius, so that no list crosses between them.

  clump A  T < 0 on every particle: every sound speed is NaN, hence every Pi and every viscous sum - every row of
           pass 3 is settled, and 512 consecutive rows of the blob order hold at least three whole blobs of 128
  clump B  healthy
  clump C  healthy but for ONE particle with T < 0 (the "bad" one): its neighbours' Pi is NaN, and the viscous sums of
           their neighbours - mixed blobs, mixed waves, rows whose own m Pi is finite beside a NaN neighbour

variant "centre"  the bad particle is the one nearest to the centre of C
        "last"    the bad particle is the farthest neighbour (rank K - 1) of at least one row: that row's sum turns NaN
                  in its last batch
        "self"    the bad particle sits beside C, outside every other particle's list: it is the rank-0 entry of its own
                  list and nothing else
        "dust"    "centre", with every fifth particle of A and C a dust particle (particle_type 2)
"""
import numpy as np

import sph_code_amd.ics as ics
from oracle import sph_oracle as orc

N_CLUMP = 512
RADIUS = 0.625e6 * ics.AU
CENTRES = np.array([[0., 0., 0.], [12., 0., 0.], [0., 12., 0.]]) * RADIUS
KS = (7, 33, 40)
VARIANTS = ("centre", "last", "self", "dust")
A, B, C = (slice(q * N_CLUMP, (q + 1) * N_CLUMP) for q in range(3))
# a step so short that the clumps stay put: 1e3 m/s x FIXED_DT = 1e-5 of the mean distance between neighbours
FIXED_DT = 1.0e9


def _clump(rs, n):
    u = rs.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    return u * (rs.rand(n) ** (1. / 3.))[:, None] * RADIUS


def knn(points, K):
    """The exact lists (oracle, eps = 0): rank 0 is the particle itself."""
    idx, _, _, _, h = orc.neighbors(points, np.inf, K, eps=0.0)
    return idx, h


def make_case(variant, K, clumps="ABC", seed=4711):
    """-> (state dict as sph_code_amd.ics builds them, index of the bad particle or None).  clumps: which of the three
    the state holds ("B": the healthy clump alone, 512 particles)."""
    assert variant in VARIANTS and set(clumps) <= set("ABC")
    rs = np.random.RandomState(seed)
    pts = np.concatenate([_clump(rs, N_CLUMP) + c for c in CENTRES])
    n = len(pts)
    vel = rs.normal(size=(n, 3)) * 1000.
    T = 10. * (1. + rs.rand(n))
    mass = np.full(n, 0.4 * ics.SOLAR / 715.)
    ptype = np.zeros(n)
    f_un = np.tile(ics.F_GAS, (n, 1))
    T[A] = -T[A]
    bad = None
    if "C" in clumps:
        c0 = C.start
        if variant in ("centre", "dust"):
            bad = c0 + int(np.argmin(np.linalg.norm(pts[C] - CENTRES[2], axis=1)))
        elif variant == "last":
            idx, _ = knn(pts, K)
            bad = int(idx[c0 + 100, K - 1])              # the farthest neighbour of row c0 + 100 (and of whoever else)
            assert C.start <= bad < C.stop
        else:
            # beside the clump: 2.5 radii from its centre - nearer to C than to anything else, further from every
            # particle of C than that particle's K nearest
            bad = c0
            pts[bad] = CENTRES[2] + np.array([0., 0., 2.5]) * RADIUS
        T[bad] = -abs(T[bad])
    if variant == "dust":
        for s in (A, C):
            d = np.arange(s.start + 3, s.stop, 5)
            d = d[d != bad]
            ptype[d] = 2.
            mass[d] = ics.DUST_MASS
            f_un[d] = ics.F_DUST
    keep = np.concatenate([np.arange(s.start, s.stop) for q, s in zip("ABC", (A, B, C)) if q in clumps])
    st = ics._finish(pts[keep], vel[keep], mass[keep], T[keep], ptype=ptype[keep], f_un=f_un[keep])
    if clumps != "ABC":
        bad = None if bad is None or bad not in keep else int(np.searchsorted(keep, bad))
    return st, bad


def hydro_args_of(state, idx, h):
    """Positional arguments of hydro_update in the reference's order (nsc:556)."""
    return (idx, state["points"], state["mass"], h, state["f_un"], state["particle_type"], state["T"],
            state["mu_array"], state["gamma_array"], state["velocities"])
