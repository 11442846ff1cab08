#!/usr/bin/env python3
"""Generate tests/golden/arb_<case>.npz: the reference's arbitrary-point samplers (nsc:1422-1527) on seeded points.

CONTAINER-ONLY TOOL, a no-op (exit 0 with a message) where the reference is absent.  It loads the reference through
make_golden.load_reference (an in-memory transform; no reference text is stored) and calls its own functions.  The
particles come from the existing fixtures <case>.npz (not duplicated here): sizes = nb_h, d = loop_d.

Per case: 384 seeded points over 1.1 x the cloud's extent, 64 points exactly on particles, 64 points farther than
R = max(sizes) outside the bounding box; n_part seeded positive; photoionization seeded with a few NaNs.  Stored:
  ref_*     the reference's own neighbors_arb list (eps = 0.1), int32 CSR, and its five outputs for that list
  exact_*   SciPy's eps = 0 list from the same kind of tree with the same radius, and the reference's outputs for it

Usage:  python tests/golden/make_golden_arb.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, load_reference  # noqa: E402

CASES = [("sphere_dust_n2048_k40", 4101), ("cube_gas_n2048_k40", 4102), ("condensed_n1024_k40", 4103)]
N_RANDOM, N_ON, N_FAR = 384, 64, 64
FIELDS = ("density", "dust_density", "temperature", "dust_temperature", "photoionization")


def csr32(rows):
    lens = np.array([len(r) for r in rows], dtype=np.int64)
    row_start = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(lens, out=row_start[1:])
    members = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows]) if row_start[-1] else np.zeros(0, np.int64)
    return row_start.astype(np.int32), members.astype(np.int32)


def make(nsc, case, seed):
    from scipy import spatial
    g = dict(np.load(os.path.join(HERE, case + ".npz"), allow_pickle=False))
    pts, mass, ptype, T, sizes = g["points"], g["mass"], g["particle_type"], g["T"], g["nb_h"]
    n = pts.shape[0]
    nsc.d = float(g["loop_d"])
    rs = np.random.RandomState(seed)
    R = float(np.max(sizes))
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    q_rand = mid + (rs.rand(N_RANDOM, 3) * 2.0 - 1.0) * 1.1 * half
    q_on = pts[rs.choice(n, N_ON, replace=False)].copy()
    # beyond R from the box: pushed out along one axis by R x (1.5 .. 3), either side
    q_far = mid + (rs.rand(N_FAR, 3) * 2.0 - 1.0) * half
    ax = rs.randint(0, 3, N_FAR)
    side = rs.randint(0, 2, N_FAR) * 2 - 1
    push = R * (1.5 + 1.5 * rs.rand(N_FAR))
    q_far[np.arange(N_FAR), ax] = np.where(side > 0, hi[ax] + push, lo[ax] - push)
    q = np.ascontiguousarray(np.concatenate([q_rand, q_on, q_far]))
    n_part = 10.0 ** rs.uniform(50.0, 54.0, n)
    photio = 10.0 ** rs.uniform(-12.0, -8.0, n)
    photio[rs.choice(n, 16, replace=False)] = np.nan
    lists = {"ref": nsc.neighbors_arb(pts, q, sizes),
             "exact": spatial.cKDTree(pts).query_ball_point(q, R, p=2, eps=0)}
    out = dict(arb_points=q, n_part=n_part, photoionization=photio, radius=np.float64(R),
               n_random=np.int64(N_RANDOM), n_on=np.int64(N_ON), n_far=np.int64(N_FAR))
    for tag, narb in lists.items():
        narb = [list(r) for r in narb]
        out[tag + "_row_start"], out[tag + "_members"] = csr32(narb)
        with np.errstate(all="ignore"):
            out[tag + "_density"] = np.asarray(nsc.density_arb(pts, q, mass, ptype, narb), dtype=np.float64)
            out[tag + "_dust_density"] = np.asarray(nsc.dust_density_arb(pts, q, mass, ptype, sizes, narb), dtype=np.float64)
            out[tag + "_temperature"] = np.asarray(nsc.temperature_arb(pts, q, mass, ptype, T, narb), dtype=np.float64)
            out[tag + "_dust_temperature"] = np.asarray(nsc.dust_temperature_arb(pts, q, mass, ptype, sizes, T, narb),
                                                        dtype=np.float64)
            out[tag + "_photoionization"] = np.asarray(nsc.photoionization_arb(pts, q, mass, n_part, photio, ptype, narb),
                                                       dtype=np.float64)
    path = os.path.join(HERE, "arb_" + case + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("%s: %d points, ref list %d, exact list %d members, %d bytes" % (
        path, q.shape[0], out["ref_members"].size, out["exact_members"].size, size))
    assert size <= 1000000, "fixture over the size limit: lower the point count"


def main():
    if not os.path.exists(REF):
        print("reference not present: nothing to do")
        return 0
    nsc = load_reference(False)
    for case, seed in CASES:
        make(nsc, case, seed)
    return 0


if __name__ == "__main__":
    sys.exit(main())
