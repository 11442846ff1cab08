"""The cool_<case>.npz fixtures joined with the particle fixtures they were made from, and cool_oracle's results on them,
computed once per case and shared by the CPU and GPU tests (treat what comes back as read-only)."""
import functools
import os

import numpy as np

import cool_oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("sphere_dust_n2048_k40", "condensed_n1024_k40")


@functools.lru_cache(maxsize=None)
def load(case):
    """-> dict: positions, particle_type, masses, sizes, neighbor (the particle fixture), f_un, mu_array, T, dt, d and the
    constants (the cool fixture), ref_<name> = the reference's results, ref_row_num_e, ref_row_contributes."""
    g = np.load(os.path.join(GOLDEN, case + ".npz"), allow_pickle=False)
    r = np.load(os.path.join(GOLDEN, "cool_" + case + ".npz"), allow_pickle=False)
    out = dict(positions=g["points"], particle_type=g["particle_type"], masses=g["mass"], sizes=g["nb_h"],
               neighbor=g["nb_idx"].astype(np.int64), f_un=r["f_un"], mu_array=r["mu_array"], T=r["T"], dt=float(r["dt"]),
               d=float(r["d"]), k=float(r["const_k"]), m_h=float(r["const_m_h"]), m_0=float(r["const_m_0"]))
    assert out["d"] == float(g["loop_d"])
    for nm in cool_oracle.OUTPUTS + ("row_num_e", "row_contributes"):
        out["ref_" + nm] = r[nm]
    return out


def compat_args(f):
    """Positional arguments of compat.rad_cooling (the reference's signature)."""
    return (f["positions"], f["particle_type"], f["masses"], f["sizes"], np.ones(f["positions"].shape[0]), f["f_un"],
            f["neighbor"], f["mu_array"], f["T"], f["dt"])


def oracle_args(f):
    return (f["positions"], f["particle_type"], f["masses"], f["f_un"], f["neighbor"], f["mu_array"], f["T"], f["dt"], f["d"])


def constants(f):
    return dict(m_0=f["m_0"], m_h=f["m_h"], k=f["k"])


@functools.lru_cache(maxsize=None)
def oracle(case):
    f = load(case)
    return cool_oracle.cooling(*oracle_args(f), **constants(f))


@functools.lru_cache(maxsize=None)
def _knn(n, seed):
    """Seeded positions and every particle's others by distance (column 0 = self), once per (n, seed)."""
    pos = np.random.RandomState(seed).rand(n, 3) * 3e16
    d2 = np.sum((pos[:, None, :] - pos[None, :, :]) ** 2, axis=2)
    d2[np.arange(n), np.arange(n)] = -1.0
    order = np.argsort(d2, axis=1, kind="stable")[:, :65]
    return pos, order, np.sqrt(np.maximum(np.take_along_axis(d2, order, axis=1), 0.0))


@functools.lru_cache(maxsize=None)
def _knn_tree(n, seed):
    """_knn's positions and lists from a k-d tree (scipy.spatial.cKDTree): no (n, n) matrix, so n may be tens of thousands.
    Column 0 = self; an exact tie may come in another order than _knn's stable sort gives (the list is an input)."""
    from scipy.spatial import cKDTree
    pos = np.random.RandomState(seed).rand(n, 3) * 3e16
    dist, order = cKDTree(pos).query(pos, k=min(65, n))
    dist, order = dist.reshape(n, -1), order.reshape(n, -1).astype(np.int64)
    assert np.array_equal(order[:, 0], np.arange(n))            # (no two seeded positions coincide)
    return pos, order, dist


def cloud(n, K, seed, dust=0.1, stars=0.02, neutral=False, tree=False):
    """A small seeded cloud with an exact kNN list (column 0 = self; entries equal to n where n <= K) and an ionised
    composition -> dict of compat.rad_cooling's arguments by name, and d.  tree=True: the list from _knn_tree (any n)."""
    pos, order, dist = _knn_tree(n, seed) if tree else _knn(n, seed)
    rs = np.random.RandomState(seed + 1000)
    pt = np.zeros(n)
    u = rs.rand(n)
    pt[u < dust] = 2.0
    pt[(u >= dust) & (u < dust + stars)] = 1.0
    m = 1e30 * (1.0 + 0.25 * rs.rand(n))
    S = 15
    f = np.zeros((n, S))
    f[:, 0] = rs.uniform(0.1, 0.5, n); f[:, 2] = rs.uniform(0.1, 0.5, n); f[:, 1] = 0.14
    if not neutral:
        f[:, 3] = rs.uniform(0.0, 0.3, n); f[:, 4] = rs.uniform(0.0, 0.05, n); f[:, 5] = f[:, 3] + f[:, 4]
    f /= np.sum(f, axis=1)[:, None]
    f[pt == 2.0] = np.array([0.0] * 7 + [0.125] * 8)
    f[::17, 5] = 0.0
    T = 10.0 ** rs.uniform(1.0, 4.5, n)
    mu = 1.0 + rs.rand(n)
    kk = min(K, n)
    nb = np.full((n, K), n, dtype=np.int64)
    nb[:, :kk] = order[:, :kk]
    # d: h(m) = (m/m_0)^(1/3) d about the distance to the min(K - 1, 12)-th neighbour: pairs fall on both sides of it
    r = float(np.median(dist[:, min(kk - 1, 12)])) if kk > 1 else 1e15
    d = float(max(r, 1e14) / np.median((m / cool_oracle.M_0) ** (1.0 / 3.0)))
    return dict(positions=pos.copy(), particle_type=pt, masses=m, sizes=np.ones(n), cross_array=np.ones(n), f_un=f,
                neighbor=nb, mu_array=mu, T=T, dt=7.9e12, d=d)


def cloud_compat_args(c):
    return (c["positions"], c["particle_type"], c["masses"], c["sizes"], c["cross_array"], c["f_un"], c["neighbor"],
            c["mu_array"], c["T"], c["dt"])


def cloud_oracle(c):
    return cool_oracle.cooling(c["positions"], c["particle_type"], c["masses"], c["f_un"], c["neighbor"], c["mu_array"],
                               c["T"], c["dt"], c["d"])
