"""Input sets of the supernova_impulse tests (tests/test_sn_cpu.py checks their conditions on the restatement,
tests/test_gpu_sn.py runs the library on them), and the committed fixture tests/golden/sn_sphere_dust_n2048_k40.npz."""
import functools
import os

import numpy as np

import sn_oracle
from conftest import GOLDEN, load_golden

M = sn_oracle.MASS_DISPLACED
CASE = "sphere_dust_n2048_k40"


@functools.lru_cache(maxsize=None)
def golden():
    """The committed fixture with the positions and types of the case it was drawn on."""
    g = load_golden(CASE)
    f = dict(np.load(os.path.join(GOLDEN, "sn_" + CASE + ".npz"), allow_pickle=False))
    f["points"] = np.array(g["points"], dtype=np.float64)
    f["particle_type"] = np.array(g["particle_type"], dtype=np.float64)
    f["velocities"] = np.array(g["velocities"], dtype=np.float64)
    return f


def cloud(n, seed, n_stars=3, select=None):
    """A mixed cloud, gas, dust and stars interleaved at random: about two thirds gas, whose masses U(0.5, 1.5) M / select
    let about `select` rows reach the boundary (default: a third of the gas); n_stars star rows, the first ones drawn near
    the centre (their selections overlap)."""
    rs = np.random.RandomState(seed)
    pts = rs.normal(size=(n, 3)) * 3.0e16
    pt = rs.choice([0.0, 0.0, 2.0], size=n)
    stars = np.sort(rs.choice(n, n_stars, replace=False)).astype(np.int64)
    pt[stars] = 1.0
    pts[stars] = rs.normal(size=(n_stars, 3)) * 3.0e15
    n_gas = int(np.sum(pt == 0))
    select = n_gas / 3.0 if select is None else select
    m = rs.uniform(0.5, 1.5, n) * M / select
    m[pt == 1] = 20.0 * sn_oracle.SOLAR_MASS
    vel = rs.normal(size=(n, 3)) * 1.0e3
    return dict(points=pts, masses=m, ptypes=pt, stars=stars, velocities=vel)


def rim(n, seed):
    """... with one star only, moved out to the rim of the cloud."""
    c = cloud(n, seed, n_stars=1)
    r = np.sqrt(np.sum(c["points"] ** 2, axis=1))
    c["points"][c["stars"][0]] = c["points"][np.argmax(r)] * 1.01
    return c


def heavy_first(n, seed):
    """The gas row nearest to the star alone weighs more than M: nothing is selected, vel = inf."""
    c = cloud(n, seed, n_stars=1)
    g, _ = sn_oracle.candidates(c["points"], c["ptypes"], int(c["stars"][0]))
    c["masses"][g[0]] = 2.0 * M
    return c


def light(n, seed, n_stars=1):
    """All the gas together weighs less than M: every gas row is selected."""
    c = cloud(n, seed, n_stars=n_stars)
    c["masses"][c["ptypes"] == 0] *= 1.0e-6
    return c


def with_nan(c, row_rank=5):
    """... a gas row near the star with a NaN coordinate: its distance orders last."""
    g, _ = sn_oracle.candidates(c["points"], c["ptypes"], int(c["stars"][0]))
    c["points"][g[row_rank], 1] = np.nan
    c["nan_row"] = int(g[row_rank])
    return c


def coincident(n, seed):
    """A gas row at the star's own position: distance 0, NaN kicks (0 / 0), counted."""
    c = cloud(n, seed, n_stars=1)
    g, _ = sn_oracle.candidates(c["points"], c["ptypes"], int(c["stars"][0]))
    c["points"][g[3]] = c["points"][c["stars"][0]]
    c["zero_row"] = int(g[3])
    return c


def mirrored(pairs=400, seed=811, selected=99):
    """The star (row 0) at the origin, `pairs` gas points p and their mirror images -p - at bit-equal squared distance -
    the images in another random order behind them, dust rows in between; equal masses M / (selected + 0.5), so exactly
    `selected` rows are selected: an odd number, the boundary falls INSIDE a pair."""
    rs = np.random.RandomState(seed)
    p = rs.normal(size=(pairs, 3))
    perm = rs.permutation(pairs)
    dust = rs.normal(size=(50, 3))
    pts = np.vstack([np.zeros((1, 3)), p, dust, -p[perm]])
    pt = np.concatenate([[1.0], np.zeros(pairs), np.full(50, 2.0), np.zeros(pairs)])
    n = pts.shape[0]
    m = np.full(n, M / (selected + 0.5))
    mirror = np.full(n, -1, dtype=np.int64)
    mirror[1 + perm] = 1 + pairs + 50 + np.arange(pairs)
    mirror[1 + pairs + 50 + np.arange(pairs)] = 1 + perm
    vel = rs.normal(size=(n, 3))
    return dict(points=pts, masses=m, ptypes=pt, stars=np.array([0], dtype=np.int64), velocities=vel, mirror=mirror)


def widening(seed=977):
    """Light rows near, heavy rows far, and ten rows of NEGATIVE mass nearest of all: the near rows' positive masses add up
    to 1.2 M - a bound over them seems enough - but the running sum starts at -0.5 M and ends the near group at 0.7 M: the
    boundary lies among the far rows, 1e4 times as far away (another key bin at the first level)."""
    rs = np.random.RandomState(seed)
    star = np.zeros((1, 3))
    neg = rs.normal(size=(10, 3)) * 0.01
    near = rs.normal(size=(300, 3))
    near += np.sign(near) * 0.1
    far = rs.normal(size=(200, 3)) * 1.0e4
    far += np.sign(far) * 1.0e3
    dust = rs.normal(size=(40, 3))
    pts = np.vstack([star, far, dust, near, neg])
    pt = np.concatenate([[1.0], np.zeros(200), np.full(40, 2.0), np.zeros(310)])
    m = np.concatenate([[20.0 * sn_oracle.SOLAR_MASS], np.full(200, M / 12.0), np.full(40, M), np.full(300, M / 250.0),
                        np.full(10, -M / 20.0)])
    m[1:201] *= rs.uniform(0.9, 1.1, 200)
    vel = rs.normal(size=(pts.shape[0], 3))
    return dict(points=pts, masses=m, ptypes=pt, stars=np.array([0], dtype=np.int64), velocities=vel)


def args(c):
    return c["points"], c["masses"], c["stars"], c["ptypes"], c["velocities"]


def same(a, b):
    """Bit for bit, a NaN equal to any NaN (0 / 0 has no payload to agree on)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))
