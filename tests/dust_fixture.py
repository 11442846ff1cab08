"""The dust_<case>.npz fixture joined with the particle fixture it was made from, the input sets the dust tests share,
and dust_oracle's results on them, computed once and shared by the CPU and GPU tests (treat what comes back as
read-only)."""
import functools
import os

import numpy as np

import cool_fixture
import dust_oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASE = "sphere_dust_n2048_k40"
ARGS = ("points", "velocities", "neighbor", "mass", "f_un", "mu_array", "sizes", "densities", "particle_type")
OPTS = ("crit_mass", "critical_density", "species_curve", "guard")
SLACK = 1e6          # every decision's margin over the bound's relative size there (dust_oracle)
# the small shapes of the GPU tests: N around the workgroup size, more than one workgroup, K + 1
CLOUD_N = (255, 256, 257, 2049)
CLOUD_K = (1, 7, 40, 64)
CLOUD_S = (8, 15, 32)


@functools.lru_cache(maxsize=None)
def load():
    """-> dict of supernova_destruction's arguments by name (ARGS), crit_mass, critical_density, amu, and
    ref_frac_destruction, ref_frac_reuptake = the reference's results."""
    g = np.load(os.path.join(GOLDEN, CASE + ".npz"), allow_pickle=False)
    r = np.load(os.path.join(GOLDEN, "dust_" + CASE + ".npz"), allow_pickle=False)
    out = dict(points=g["points"], particle_type=g["particle_type"], neighbor=g["nb_idx"].astype(np.int64),
               velocities=r["velocities"], mass=r["mass"], f_un=r["f_un"], mu_array=r["mu_array"], sizes=r["sizes"],
               densities=r["densities"], crit_mass=float(r["crit_mass"]), critical_density=float(r["critical_density"]),
               amu=float(r["const_amu"]), guard="count", species_curve=None)
    for nm in dust_oracle.OUTPUTS:
        out["ref_" + nm] = r[nm]
    return out


@functools.lru_cache(maxsize=None)
def fraction_set():
    """The fixture with densities = critical_density 10^U(-1, 2.5), for guard="fraction": the reference's natural range
    never reaches the cap at 0.99, this one does, and a grain's accumulated loss reaches its atom count."""
    f = dict(load())
    rs = np.random.RandomState(11)
    f["densities"] = f["critical_density"] * 10.0 ** rs.uniform(-1.0, 2.5, f["points"].shape[0])
    f["guard"] = "fraction"
    return f


def args(f):
    return tuple(f[nm] for nm in ARGS)


def opts(f):
    return {nm: f[nm] for nm in OPTS}


def run_oracle(f):
    return dust_oracle.destruction(*args(f), amu=f.get("amu", dust_oracle.AMU), **opts(f))


@functools.lru_cache(maxsize=None)
def oracle(which):
    return run_oracle(load() if which == "count" else fraction_set())


def cloud(n, K, S, seed, guard="fraction", dust=0.15, stars=0.02):
    """A small seeded cloud with an exact kNN list (column 0 = self; entries equal to n where n <= K): dust of drawn masses
    (crit_mass their median), sizes and compositions, relative speeds on both sides of the curves' last knot, densities
    that put losses on both sides of the guard's limit (and, for guard="fraction", of the cap)."""
    pos, order, dist = cool_fixture._knn(n, seed)
    rs = np.random.RandomState(seed + 2000)
    pt = np.zeros(n)
    u = rs.rand(n)
    pt[u < dust] = 2.0
    pt[(u >= dust) & (u < dust + stars)] = 1.0
    isd = pt == 2.0
    m = 1e26 * (1.0 + rs.rand(n))
    crit_mass = float(np.median(m[isd])) if isd.any() else 1e26
    f = np.zeros((n, S))
    f[:, 0] = 0.86; f[:, 1] = 0.14
    lo = min(6, S - 2)
    fd = np.zeros((n, S)); fd[:, lo:] = rs.uniform(0.0, 1.0, (n, S - lo))
    fd /= np.sum(fd, axis=1)[:, None]
    f[isd] = fd[isd]
    mu = 1.0 + 50.0 * rs.rand(n)
    vel = rs.normal(0.0, 7e4, (n, 3))
    kk = min(K, n)
    nb = np.full((n, K), n, dtype=np.int64)
    nb[:, :kk] = order[:, :kk]
    # sizes about the distance to the min(K - 1, 6)-th neighbour, times U(0.7, 1.6): never a neighbour's distance itself
    col = min(kk - 1, 6)
    sizes = (dist[:, col] if col > 0 else np.full(n, 1e15)) * rs.uniform(0.7, 1.6, n)
    cd = dust_oracle.CRITICAL_DENSITY
    if guard == "fraction":
        dens = cd * 10.0 ** rs.uniform(-1.0, 2.5, n)
    else:
        dens = cd * 10.0 ** rs.uniform(-2.0, 2.0, n) / (1e26 / (25.0 * dust_oracle.AMU))
    return dict(points=pos.copy(), velocities=vel, neighbor=nb, mass=m, f_un=f, mu_array=mu, sizes=sizes, densities=dens,
                particle_type=pt, crit_mass=crit_mass, critical_density=cd, species_curve=None, guard=guard)


def shape_specs(K):
    """The clouds of one K: every N of CLOUD_N and K + 1, S and the guard cycling -> [(name, arguments of cloud)]."""
    out = []
    for a, n in enumerate(sorted(set(CLOUD_N + (K + 1,)))):
        S = CLOUD_S[(a + K) % 3]
        out.append(("n=%d K=%d S=%d" % (n, K, S), (n, K, S, 300 + K + a, ("fraction", "count")[a % 2])))
    return out


def shape_clouds(K):
    return [(name, cloud(*spec)) for name, spec in shape_specs(K)]


SHORT = ((5, 7), (7, 7), (40, 64))


def short_cloud(n, K):
    """N <= K: entries equal to N contribute nothing."""
    return cloud(n, K, 15, 40 + n, dust=0.4, stars=0.0)


def hub(guard):
    """One dust grain (particle 0) in the rows of 600 gas particles on a shell round it - a reverse slice longer than a
    workgroup - each taking a few per cent of the limit, so the guard flips somewhere inside the slice."""
    n, K, S = 601, 3, 15
    rs = np.random.RandomState(77)
    u = rs.normal(size=(n, 3))
    u /= np.sqrt(np.sum(u ** 2, axis=1))[:, None]
    pos = 1e16 * u * rs.uniform(0.3, 0.9, n)[:, None]
    pos[0] = 0.0
    pt = np.zeros(n); pt[0] = 2.0
    j = np.arange(n)
    nb = np.stack([j, np.zeros(n, np.int64), 1 + j % (n - 1)], axis=1)
    nb[0] = [0, 1, 2]
    m = np.full(n, 1e26); m[0] = 3e26
    f = np.zeros((n, S)); f[:, 0] = 0.86; f[:, 1] = 0.14
    f[0] = 0.0; f[0, 7:13] = rs.uniform(0.5, 1.5, 6); f[0] /= f[0].sum()
    mu = np.full(n, 2.0); mu[0] = 40.0
    sizes = np.full(n, 1.5e16)
    vel = rs.normal(0.0, 6e4, (n, 3)); vel[0] = 0.0
    cd = dust_oracle.CRITICAL_DENSITY
    N0 = m[0] / (mu[0] * dust_oracle.AMU)
    dens = cd * rs.uniform(0.5, 1.5, n) * (1.0 if guard == "fraction" else 1.0 / N0)
    return dict(points=pos, velocities=vel, neighbor=nb, mass=m, f_un=f, mu_array=mu, sizes=sizes, densities=dens,
                particle_type=pt, crit_mass=1e26, critical_density=cd, species_curve=None, guard=guard)


OWN_SELECTOR = (0, 2, 0, 0, 0, 0, 0, 1, 1, 2, 2, 0, 0, 1, 2)


def extra(name):
    """Clouds run with other options than the defaults."""
    if name == "own selector":
        return dict(cloud(257, 7, 15, 5), species_curve=np.array(OWN_SELECTOR, dtype=np.int32))
    f = cloud(257, 7, 15, 6)
    return {"every grain above crit_mass": dict(f, crit_mass=0.0), "no grain above crit_mass": dict(f, crit_mass=1e40),
            "another critical density": dict(f, critical_density=3.0 * f["critical_density"])}[name]


EXTRAS = ("own selector", "every grain above crit_mass", "no grain above crit_mass", "another critical density")


def input_sets():
    """Every input set whose regime counts a GPU test compares with the restatement's -> {name: callable that builds it}
    (building is left to the test: collecting the module costs nothing)."""
    out = {"fixture": load, "fixture, fraction": fraction_set}
    for K in CLOUD_K:
        for name, spec in shape_specs(K):
            out[name] = functools.partial(cloud, *spec)
    for n, K in SHORT:
        out["short n=%d K=%d" % (n, K)] = functools.partial(short_cloud, n, K)
    for g in ("count", "fraction"):
        out["hub, " + g] = functools.partial(hub, g)
    for name in EXTRAS:
        out[name] = functools.partial(extra, name)
    out["no dust"] = functools.partial(cloud, 300, 7, 15, 8, dust=0.0)
    out["side call"] = functools.partial(cloud, 300, 40, 15, 32)
    return out
