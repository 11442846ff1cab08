"""The inputs of the projected maps' tests, stated once: tests/test_gpu_map.py runs the library on each and
tests/test_map_cpu.py checks on each that no (particle, pixel) pair sits on the edge of a support (map_oracle's "edge" and
"box_edge" are 0), so that the counts of the two sides may be compared for equality.  The restatement of a case is computed
once per process (reference())."""
import os

import numpy as np

import map_oracle as mo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("sphere_dust_n2048_k40", "cube_gas_n2048_k40", "condensed_n1024_k40")
NPIX = ((1, 1), (15, 15), (16, 16), (17, 17), (33, 65), (65, 33))
AXES = ((0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1))
M_0 = 10 ** 1.5 * 1.989e30           # compat.m_0 (test_gpu_map.py checks that it is)
_fix, _ref = {}, {}


def fixture(name):
    """points, mass, particle_type, sizes (nb_h), T and d (loop_d) of a golden fixture."""
    if name not in _fix:
        g = np.load(os.path.join(GOLDEN, name + ".npz"))
        _fix[name] = dict(points=g["points"].astype(np.float64), mass=g["mass"].astype(np.float64),
                          particle_type=g["particle_type"].astype(np.float64), sizes=g["nb_h"].astype(np.float64),
                          T=g["T"].astype(np.float64), d=float(g["loop_d"]))
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in _fix[name].items()}


def extent(s):
    """Half-width of the window that holds the cloud: the largest |coordinate|, 10 % wider."""
    return 1.1 * float(np.max(np.abs(s["points"])))


def _case(s, axes=(1, 2), center=(0., 0.), half_width=None, npix=(17, 15), depth=None):
    hw = extent(s) if half_width is None else half_width
    hw = (float(hw), float(hw)) if np.ndim(hw) == 0 else tuple(float(x) for x in hw)
    return dict(state=s, axes=tuple(axes), center=tuple(float(x) for x in center), half_width=hw, npix=tuple(npix),
                depth=None if depth is None else tuple(float(x) for x in depth))


def _synthetic(pts, ptype, R, T=None, m=None):
    """A few rows with chosen footprints: dust rows take R as their size, gas rows the mass whose h(m) is R at d = 1."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    n = pts.shape[0]
    pt = np.broadcast_to(np.asarray(ptype, dtype=np.float64), (n,)).copy()
    R = np.broadcast_to(np.asarray(R, dtype=np.float64), (n,)).copy()
    mass = np.full(n, 2.5e30) if m is None else np.broadcast_to(np.asarray(m, dtype=np.float64), (n,)).copy()
    gas = pt == 0
    mass[gas] = M_0 * R[gas] ** 3
    return dict(points=pts, mass=mass, particle_type=pt, sizes=R.copy(), T=np.full(n, 50.) if T is None else np.asarray(T, dtype=np.float64),
                d=1.0)


def _subset(name, n, seed):
    s = fixture(name)
    rng = np.random.RandomState(seed)
    dust = np.flatnonzero(s["particle_type"] == 2)
    gas = np.flatnonzero(s["particle_type"] == 0)
    nd = min(n // 3, dust.size)
    idx = np.sort(np.concatenate((rng.choice(dust, nd, replace=False), rng.choice(gas, n - nd, replace=False))))
    return {k: (v[idx] if isinstance(v, np.ndarray) else v) for k, v in s.items()}


def build():
    """name -> case (state, axes, center, half_width, npix, depth)."""
    c = {}
    for f in FIXTURES:
        for nu, nv in NPIX:
            c["%s-%dx%d" % (f, nu, nv)] = _case(fixture(f), npix=(nu, nv))
    sd = FIXTURES[0]
    for au, av in AXES:
        c["axes-%d%d" % (au, av)] = _case(fixture(sd), axes=(au, av), half_width=(extent(fixture(sd)), 0.8 * extent(fixture(sd))))
    e = extent(fixture(sd))
    c["zoom20"] = _case(fixture(sd), half_width=e / 20)
    c["beside"] = _case(fixture(sd), center=(40 * e, 0.), half_width=e)
    c["half-off"] = _case(fixture(sd), center=(e, -0.3 * e), half_width=e, npix=(33, 17))
    s = fixture(sd)
    x = np.sort(s["points"][:, 0])
    c["slab-lo-at-a-particle"] = _case(s, depth=(x[700], x[1500] + 0.5 * (x[1501] - x[1500])))
    c["slab-hi-at-a-particle"] = _case(s, depth=(x[700] - 0.5 * (x[700] - x[699]), x[1500]))
    for n in (1, 2, 257):
        c["subset-n%d" % n] = _case(_subset(sd, n, 3 + n), npix=(17, 17))
    c["one-dust-row"] = _case(_synthetic([[0., 0.1, -0.2]], 2, 0.7), half_width=1.0, npix=(17, 17))
    st = _subset(sd, 64, 9)
    st["particle_type"][:] = 1.0
    c["all-stars"] = _case(st)
    bad = _subset(sd, 300, 11)
    e_bad = extent(bad)
    bad["points"][5, 0] = np.nan              # the line of sight's coordinate of axes (1, 2)
    bad["points"][17, 2] = np.nan
    bad["points"][40, 1] = np.inf
    bad["mass"][77] = np.nan
    k = int(np.flatnonzero(bad["particle_type"] == 2)[3])
    bad["sizes"][k] = 0.0                     # R = 0
    k2 = int(np.flatnonzero(bad["particle_type"] == 2)[5])
    bad["sizes"][k2] = -bad["sizes"][k2]
    st1 = int(np.flatnonzero(bad["particle_type"] == 0)[0])
    bad["particle_type"][st1] = 1.0           # a star with a NaN coordinate is no row of the maps: not skipped either
    bad["points"][st1, 1] = np.nan
    c["bad-rows"] = _case(bad, half_width=e_bad, npix=(33, 17))
    # 16 pixels of width 1/8 on [-1, 1): centres at odd multiples of 1/16.  A disc of radius 0.05 at the origin lies between
    # four centres; beside it a disc that holds exactly one centre, and one whose position IS a pixel centre, bit for bit.
    c["between-centres"] = _case(_synthetic([[0., 0., 0.], [0.3, 0.0625 + 0.01, 0.0625 - 0.02], [0., 0.4, 0.4]], [2, 0, 2], [0.05, 0.05, 0.05]),
                                 half_width=1.0, npix=(16, 16))
    uu = mo.centres(0.25, 1.5, 17)
    vv = mo.centres(-0.5, 0.75, 15)
    c["on-a-centre"] = _case(_synthetic([[0.1, uu[5], vv[9]], [0.2, uu[16], vv[0]], [0.3, uu[0], vv[14]]], [0, 2, 0], [0.33, 0.45, 0.21]),
                             center=(0.25, -0.5), half_width=(1.5, 0.75), npix=(17, 15))
    rng = np.random.RandomState(21)
    n = 3000
    line = np.zeros((n, 3))
    line[:, 0] = rng.uniform(-5, 5, n)
    line[:, 1], line[:, 2] = 0.137, -0.291
    c["long-list"] = _case(_synthetic(line, rng.choice([0., 2.], n), rng.uniform(0.2, 0.9, n), T=rng.uniform(10, 1e4, n)),
                           half_width=1.0, npix=(20, 18))
    neg = fixture(sd)
    neg["T"][::3] = -neg["T"][::3]
    neg["T"][np.flatnonzero(neg["particle_type"] == 2)[::2]] *= -1.0
    c["negative-T"] = _case(neg, npix=(33, 17))
    c["gas-only-and-dust-only-pixels"] = _case(_synthetic([[0., -0.5, 0.], [0., 0.5, 0.], [0., -0.5, 0.05]], [0, 2, 0], [0.3, 0.3, 0.25],
                                                          T=[100., 20., -40.]), half_width=1.0, npix=(32, 8))
    return c


CASES = build()


def reference(name):
    if name not in _ref:
        k = CASES[name]
        s = k["state"]
        _ref[name] = mo.project(s["points"], s["mass"], s["particle_type"], s["sizes"], s["T"], s["d"], M_0, axes=k["axes"],
                                center=k["center"], half_width=k["half_width"], npix=k["npix"], depth=k["depth"])
    return _ref[name]
