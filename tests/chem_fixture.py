"""The chem_<case>.npz fixture joined with the particle fixture it was made from, the seeded input sets the chem tests
share, and chem_oracle's results on them, computed once per set and shared by the CPU and GPU tests (treat what comes
back as read-only).  Every set is held to the margin condition of chem_oracle (`slack` >= SLACK for every kind of
decision) by tests/test_chem_cpu.py; a set that fails it changes its seed."""
import functools
import os

import numpy as np

import chem_oracle
import cool_fixture

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASE = "sphere_dust_n2048_k40"
ARGS = ("points", "neighbor", "mass", "f_un", "mu_array", "sizes", "T", "particle_type")
TABLES = ("mu_specie", "mineral_densities", "sputtering_yields")
SLACK = 1e6          # every decision's margin over the bound's size there (chem_oracle)
DT_0 = chem_oracle.DT_0
CLOUD_N = (255, 256, 257, 2049)
CLOUD_K = (1, 7, 40, 64)
CLOUD_S = (7, 15, 32)


@functools.lru_cache(maxsize=None)
def load():
    """-> dict of chemisputtering_2's arguments by name (ARGS), d, dt, the tables, and ref_mass_new, ref_f_un_new = the
    reference's results."""
    g = np.load(os.path.join(GOLDEN, CASE + ".npz"), allow_pickle=False)
    r = np.load(os.path.join(GOLDEN, "chem_" + CASE + ".npz"), allow_pickle=False)
    out = dict(points=g["points"], particle_type=g["particle_type"], neighbor=g["nb_idx"].astype(np.int64), mass=g["mass"],
               T=g["T"], f_un=r["f_un"], mu_array=r["mu_array"], sizes=r["sizes"], d=float(r["d"]), dt=float(r["dt"]),
               mu_specie=r["mu_specie"], mineral_densities=r["mineral_densities"], sputtering_yields=r["sputtering_yields"],
               mrn=r["mrn"], k_B=float(r["const_k"]), amu=float(r["const_amu"]), m_0=float(r["const_m_0"]))
    for nm in chem_oracle.OUTPUTS:
        out["ref_" + nm] = r[nm]
    return out


def module_dt_set():
    """The fixture at the module's dt (dt_0), every gas particle with refractory shares (a zeroed row takes the next
    row's; all twenty times the fixture's): nothing is clamped, two rounds, the dust's masses move by ~1e-5."""
    f = dict(load())
    fun = f["f_un"].copy()
    gas = np.nonzero(f["particle_type"] == 0)[0]
    zeroed = gas[np.all(fun[gas, 7:] == 0.0, axis=1)]
    donors = gas[~np.all(fun[gas, 7:] == 0.0, axis=1)]
    fun[zeroed, 7:] = fun[donors[np.arange(len(zeroed)) % len(donors)], 7:]
    fun[gas, 7:] *= 20.0
    fun /= np.sum(fun, axis=1)[:, None]
    f["f_un"] = fun
    f["mu_array"] = np.sum(fun * f["mu_specie"], axis=1) / np.sum(fun, axis=1)
    f["dt"] = DT_0
    return f


def args(f):
    return tuple(f[nm] for nm in ARGS)


def run_oracle(f, model=True):
    kw = {nm: f[nm] for nm in TABLES + ("mrn", "k_B", "amu", "m_0") if nm in f}
    return chem_oracle.sputter(*args(f), d=f["d"], dt=f["dt"], model=model, **kw)


def cloud(n, K, S, seed, dust=0.15, stars=0.02, gas=True, dt=1e6 * DT_0, negative=False, tree=False, mass=3e22):
    """A small seeded cloud with an exact kNN list (column 0 = self; entries equal to n where n <= K): gas with shares of
    H+, He+, He++ and of the columns >= 6, those of every second gas particle exactly 0 (clamp 1 at dt = 1e6 dt_0), dust
    spread over the columns >= min(7, S - 1).  gas=False: stars in the gas's place.  negative=True: one entry in eight of
    the columns >= 6, gas and dust alike, negative (clamps 2 and 3 and the closing correction)."""
    pos, order, dist = cool_fixture._knn_tree(n, seed) if tree else cool_fixture._knn(n, seed)
    rs = np.random.RandomState(seed + 3000)
    pt = np.zeros(n)
    u = rs.rand(n)
    pt[u < dust] = 2.0
    pt[(u >= dust) & (u < dust + stars)] = 1.0
    if not gas:
        pt[pt == 0.0] = 1.0
    isd = pt == 2.0
    m = mass * (1.0 + 0.25 * rs.rand(n))
    mus, dens, ys = chem_oracle.tables(S)
    f = np.zeros((n, S))
    f[:, 0] = rs.uniform(0.1, 0.5, n); f[:, 2] = rs.uniform(0.1, 0.5, n); f[:, 1] = 0.14
    f[:, 3] = rs.uniform(0.0, 0.05, n); f[:, 4] = rs.uniform(0.0, 0.01, n); f[:, 5] = rs.uniform(0.0, 0.01, n)
    f[:, 6:] = rs.uniform(0.0, 1e-4, (n, S - 6))
    f[::2, 6:] = 0.0
    f[::17, 5] = 0.0
    f /= np.sum(f, axis=1)[:, None]
    lo = min(7, S - 1)
    fd = np.zeros((n, S)); fd[:, lo:] = rs.uniform(0.05, 1.0, (n, S - lo))
    fd /= np.sum(fd, axis=1)[:, None]
    f[isd] = fd[isd]
    if negative:
        flip = rs.rand(n, S - 6) < 0.125
        f[:, 6:] = np.where(flip, -0.3 * np.abs(f[:, 6:]), f[:, 6:])
    mu = np.sum(f * mus, axis=1) / np.sum(f, axis=1)
    T = 10.0 ** rs.uniform(1.0, 4.5, n)
    kk = min(K, n)
    nb = np.full((n, K), n, dtype=np.int64)
    nb[:, :kk] = order[:, :kk]
    # d: h(m) = (m/m_0)^(1/3) d about the distance to the min(K - 1, 12)-th neighbour: pairs fall on both sides of it
    r = float(np.median(dist[:, min(kk - 1, 12)])) if kk > 1 else 1e15
    d = float(max(r, 1e14) / np.median((m / chem_oracle.M_0) ** (1.0 / 3.0)))
    sizes = (dist[:, min(kk - 1, 6)] if kk > 1 else np.full(n, 1e15)) * rs.uniform(0.7, 1.6, n)
    return dict(points=pos.copy(), neighbor=nb, mass=m, f_un=f, mu_array=mu, sizes=sizes, T=T, particle_type=pt, d=d, dt=dt,
                mu_specie=mus, mineral_densities=dens, sputtering_yields=ys)


# seeds under which the set meets the margin condition (tests/test_chem_cpu.py); searched from the first entry upward
SEEDS = {"n=255 K=7 S=32": 509, "n=257 K=7 S=15": 513, "n=2049 K=7 S=32": 517, "n=257 K=40 S=15": 544, "n=2049 K=40 S=32": 545,
         "n=255 K=64 S=32": 566, "n=257 K=64 S=15": 569, "n=2049 K=64 S=32": 570, "short n=7 K=7": 68, "negative": 26}


def shape_specs(K):
    """The clouds of one K: every N of CLOUD_N and K + 1, S cycling -> [(name, arguments of cloud)]."""
    out = []
    for a, n in enumerate(sorted(set(CLOUD_N + (K + 1,)))):
        S = CLOUD_S[(a + K) % 3]
        name = "n=%d K=%d S=%d" % (n, K, S)
        # (a third of the dust at the largest N: the margin condition is over every clamp event of a set)
        out.append((name, (n, K, S, SEEDS.get(name, 500 + K + a), 0.05 if n > 2000 else 0.15)))
    return out


def shape_clouds(K):
    return [(name, cloud(*spec)) for name, spec in shape_specs(K)]


SHORT = ((5, 7), (7, 7), (40, 64))


def short_cloud(n, K):
    """N <= K: entries equal to N contribute nothing."""
    return cloud(n, K, 15, SEEDS.get("short n=%d K=%d" % (n, K), 60 + n), dust=0.4, stars=0.0)


HUB_ROWS = 64


def hub():
    """One gas particle (0) in the list of each of 64 dust rows (1..64), and nothing else in it but the row itself: every
    row finds the hub's count of each column >= 7 too small for what it would take (clamp 1), takes 99 % of it and leaves
    1 % to the next, so row j's loss depends on row j - 1's - a chain as deep as the rows."""
    n, K, S = 1 + HUB_ROWS, 2, 15
    rs = np.random.RandomState(91)
    mus, dens, ys = chem_oracle.tables(S)
    u = rs.normal(size=(n, 3))
    u /= np.sqrt(np.sum(u ** 2, axis=1))[:, None]
    pos = 1e16 * u * rs.uniform(0.2, 0.8, n)[:, None]
    pos[0] = 0.0
    pt = np.full(n, 2.0); pt[0] = 0.0
    j = np.arange(n)
    nb = np.stack([j, np.zeros(n, np.int64)], axis=1)
    nb[0] = [0, 1]
    m = 1e26 * (1.0 + 0.25 * rs.rand(n)); m[0] = 1e23
    f = np.zeros((n, S))
    f[:, 7:] = rs.uniform(0.05, 1.0, (n, S - 7))
    f[0] = 0.0
    f[0, 0] = 0.5; f[0, 1] = 0.14; f[0, 2] = 0.3; f[0, 3] = 0.03; f[0, 4] = 0.005; f[0, 5] = 0.005
    f[0, 7:] = rs.uniform(0.2e-4, 1e-4, S - 7)
    f /= np.sum(f, axis=1)[:, None]
    mu = np.sum(f * mus, axis=1) / np.sum(f, axis=1)
    T = np.full(n, 3000.0)
    d = float(1.5e16 / (m[0] / chem_oracle.M_0) ** (1.0 / 3.0))
    sizes = np.full(n, 1.5e17) * rs.uniform(0.8, 1.2, n)             # (enters through the row's own dust density alone)
    return dict(points=pos, neighbor=nb, mass=m, f_un=f, mu_array=mu, sizes=sizes, T=T, particle_type=pt, d=d, dt=1e6 * DT_0,
                mu_specie=mus, mineral_densities=dens, sputtering_yields=ys)


def input_sets():
    """Every input set whose counts a GPU test compares with the restatement's -> {name: callable that builds it}
    (building is left to the test: collecting the module costs nothing)."""
    out = {"fixture": load, "module dt": module_dt_set}
    for K in CLOUD_K:
        for name, spec in shape_specs(K):
            out[name] = functools.partial(cloud, *spec)
    for n, K in SHORT:
        out["short n=%d K=%d" % (n, K)] = functools.partial(short_cloud, n, K)
    out["hub"] = hub
    out["negative"] = functools.partial(cloud, 300, 7, 15, SEEDS.get("negative", 21), negative=True)
    out["no dust"] = functools.partial(cloud, 300, 7, 15, 8, dust=0.0)
    out["all dust"] = functools.partial(cloud, 300, 7, 15, 9, dust=1.1)
    out["no gas"] = functools.partial(cloud, 300, 7, 15, 10, gas=False)
    out["overflow"] = functools.partial(cloud, 257, 7, 15, 12, mass=1e27)
    out["side call"] = functools.partial(cloud, 300, 40, 15, SEEDS.get("side call", 33))
    return out


@functools.lru_cache(maxsize=None)
def built(name):
    """-> (the input set, chem_oracle's result on it with the round model run), once per name."""
    f = input_sets()[name]()
    return f, run_oracle(f)
