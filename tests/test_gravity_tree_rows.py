"""Tree gravity (sphx_gravity.hip: pyramid build, per-thread walk, wave/LDS walk; monopoles and second
moments) pinned ROW BY ROW to the oracle's direct sum, in two limits whose answer does not depend on the
library's grid - the grid (origin, cell edge, every particle's cell) comes out of device reductions and
cannot be restated on the host, and one particle across a cell face moves a row by 1e-3.

1. Every source exactly once (eps >> D, D the diagonal of the true bounding box).  The pair kernel is
   d / eps^3 * (1 - 1.5 d^2 / eps^2 + ...), and the linear part of a cell's monopole is exact:
   sum m_j (x_j - x) = M (c - x).  So for ANY partition of the sources into cells, of either order,
       |tree_i - direct_i| <= (4 (D/eps)^2 + 1e-12) * sum_j |term_ij|        component by component.
   Derivation, component z, one cell (M, c) against its members, d = x_j - x, r = c - x: what is left is
   cubic, 1.5 / eps^5 * |sum m |d|^2 d_z - M |r|^2 r_z| <= 1.5 D^2 / eps^5 (sum m |d_z| + M |r_z|), and
   M |r_z| = |sum m d_z| <= sum m |d_z|: 3 (D/eps)^2 of the row's scale.  The second-order terms change
   the cubic remainder to 1.5 / eps^5 |sum m |delta|^2 delta_z|, delta = x_j - c, and
   sum m |delta_z| <= 2 sum m |d_z|: again 3 (D/eps)^2.  1e-12 is the round-off allowance of a signed sum.
   A source left out or counted twice moves a row by ~1e-4 of its scale, eight orders above the bound.

2. The multipole terms themselves.  A cluster B (mass M, inside a ball of radius b about c0) seen by
   zero-mass targets at distance d from c0, softening eps, s^2 = d^2 + eps^2.  With f = 1 / sqrt(r^2 + eps^2)
   the acceleration is a = -grad f.  Along any line r + t u (|u| = 1)
       f = 1 / sqrt(s^2 + 2 t (r.u) + t^2) = (1/s) sum_k (-t/s)^k P_k(r.u / s),
   so the k-th directional derivative is k! P_k / s^(k+1) in size, and |P_k| <= 1 on [-1, 1]: the k-th
   derivative of f, a symmetric k-linear form, has norm <= k! / s^(k+1) (its norm is attained on a single
   direction).  Expand a cell of B about its centre of mass c (delta = x_j - c, sum m delta = 0):
     order 1 leaves  sum m int_0^1 (1-t) D^3 f(r + t delta)[delta, delta, .] dt,
                     at most 1/2 * 3! / s_min^4 * sum m |delta|^2;
     order 2 leaves  at most 1/6 * 4! / s_min^5 * sum m |delta|^3.
   Every cell's centre lies in the ball, so every point r + t delta is at least d - b from the target:
   s_min >= (1 - b/d) s.  Moments about the cells' own centres are no larger than about c0:
   sum m |delta|^2 <= M b^2 = M (2b)^2 / 4, and |delta| <= 2b gives sum m |delta|^3 <= M (2b)^3 / 4.  Hence
       |a_tree - a_direct| <= C_p G M (2b)^(p+1) / s^(p+3),   C_1 = 0.75 / (1 - b/d)^4,  C_2 = 1 / (1 - b/d)^5
   for any sub-partition of B, any mixture of expanded and directly summed cells.  These constants are for
   the worst cluster and the worst cut; a random split of a round cluster stays 10 to 50 times below them.
   So that the order-1 error of every row still stands clear of the ORDER-2 bound, and a wrong coefficient
   of the second-order term does too, B is a bar (second moment M b^2 / 3 along its axis), not a ball.

The CPU tests prove both bounds on NumPy restatements of the expansion over arbitrary partitions, and that
a dropped source, a doubled source and a mutated coefficient break them; the GPU tests apply the bounds to
both kernels."""
import itertools

import numpy as np
import pytest

AU = 149597870700.0
SOLAR = 1.989e30
G = 6.67430e-11
EPS_OVER_D = 1e6
TOL_LIMIT = 4.0 / EPS_OVER_D ** 2 + 1e-12          # limit 1: 4 (D/eps)^2 + round-off
QUAD_COEF = (7.5, 1.5, 3.0)


# =================================================================================================
# NumPy restatement of a cell's expansion (CPU proofs only)
# =================================================================================================
def _expand(ps, ms, xt, e2, order, coef=QUAD_COEF):
    """Acceleration / G at the targets xt (t,3) of the sources (ps, ms) taken as ONE cell: its mass at its
    centre of mass, and for order 2 the second moments about it (the softened kernel's own expansion)."""
    M = ms.sum()
    c = (ms[:, None] * ps).sum(axis=0) / M
    r = c - xt
    s = np.sqrt((r * r).sum(axis=1) + e2)
    a = (M / s ** 3)[:, None] * r
    if order == 2:
        dl = ps - c
        S = (ms[:, None, None] * dl[:, :, None] * dl[:, None, :]).sum(axis=0)
        Sr = r @ S
        rSr = (r * Sr).sum(axis=1)
        a = a + (coef[0] * rSr / s ** 7 - coef[1] * np.trace(S) / s ** 5)[:, None] * r - coef[2] * Sr / (s ** 5)[:, None]
    return a


def _partition_sum(ps, ms, lab, xt, e2, order, coef=QUAD_COEF):
    a = np.zeros_like(xt)
    for g in np.unique(lab):
        sel = lab == g
        if ms[sel].sum() > 0.0:
            a += _expand(ps[sel], ms[sel], xt, e2, order, coef)
    return a


def _direct(p, m, eps):
    """(oracle's direct sum, sum_j |term_ij| per component)"""
    from oracle import sph_oracle as orc
    return orc.gravity_direct(p, m, eps, G=G, return_abs=True)


# =================================================================================================
# 1. the large-softening limit
# =================================================================================================
def _gauss(n, seed):
    rs = np.random.RandomState(seed)
    return rs.normal(size=(n, 3)) * 1e5 * AU, rs.uniform(0.5, 2.0, n) * 1e-3 * SOLAR


def _heavy_tail(n=5003, seed=5):
    rs = np.random.RandomState(seed)
    return rs.standard_t(2, size=(n, 3)) * 1e5 * AU, rs.uniform(0.5, 2.0, n) * 1e-3 * SOLAR


def _flat(axes, thickness, n=4001, seed=11):
    """a slab (axes = (2,)) or a line (axes = (1, 2)): those coordinates are 0, or thickness * D wide"""
    p, m = _gauss(n, seed)
    rs = np.random.RandomState(seed + 1)
    for a in axes:
        p[:, a] = 0.0
    D = np.linalg.norm(p.max(axis=0) - p.min(axis=0))
    for a in axes:
        p[:, a] = thickness * D * rs.uniform(-0.5, 0.5, n)
    return p, m


def _lattice():
    pitch = 2.0 ** 44                                # (1.8e13 m: every coordinate an exact multiple)
    ix, iy, iz = np.meshgrid(np.arange(17.0), np.arange(13.0), np.arange(11.0), indexing="ij")
    p = np.stack([ix.ravel(), iy.ravel(), iz.ravel()], axis=1) * pitch
    p = np.vstack([p, np.tile(np.array([[8.0, 6.0, 5.0]]) * pitch, (50, 1))])       # 50 on one node
    m = np.random.RandomState(17).uniform(0.5, 2.0, len(p)) * 1e-3 * SOLAR
    return p, m


def _zero_scattered():
    p, m = _gauss(3000, 23)
    m[np.random.RandomState(24).rand(3000) < 0.3] = 0.0
    return p, m


def _zero_but_one():
    p, m = _gauss(3000, 29)
    keep = m[1234]
    m[:] = 0.0
    m[1234] = keep
    return p, m


def _shifted(m_, n=5003):
    """the N = 5003 cloud 2^m_ cloud sizes from the origin (R0: the power of two >= max|x|); snapped to R0 2^-20 first, so
    that the shift is exact and the direct sum sees the differences of the cloud at the origin"""
    p, m = _gauss(n, 100 + n)
    R0 = 2.0 ** np.ceil(np.log2(np.abs(p).max()))
    p = np.round(p / (R0 * 2.0 ** -20)) * (R0 * 2.0 ** -20)
    return p + R0 * np.array([2.0 ** m_, -(2.0 ** (m_ - 1)), 2.0 ** (m_ - 2)]), m


LIMIT_CASES = {"gauss_%d" % n: (lambda n=n: _gauss(n, 100 + n)) for n in (1, 2, 63, 64, 65, 257, 1000, 5003)}
LIMIT_CASES.update({
    "heavy_tail": _heavy_tail,
    "slab": lambda: _flat((2,), 0.0),
    "line": lambda: _flat((1, 2), 0.0),
    "slab_thin": lambda: _flat((2,), 1e-9),
    "line_thin": lambda: _flat((1, 2), 1e-9),
    "lattice": _lattice,
    "zero_mass_30pc": _zero_scattered,
    "zero_mass_but_one": _zero_but_one,
    "gauss_5003_shift_20": lambda: _shifted(20),
    "gauss_5003_shift_27": lambda: _shifted(27),
})
_limit_cache = {}


def _limit_case(name):
    """(points, mass, eps, reference rows, row scales), computed once and left unchanged"""
    if name not in _limit_cache:
        p, m = LIMIT_CASES[name]()
        p = np.ascontiguousarray(p)
        m = np.ascontiguousarray(m)
        D = np.linalg.norm(p.max(axis=0) - p.min(axis=0))
        eps = EPS_OVER_D * D if D > 0.0 else 1.0                  # (one particle: nothing to soften)
        ref, scale = _direct(p, m, eps)
        for a in (p, m, ref, scale):
            a.setflags(write=False)
        _limit_cache[name] = (p, m, eps, ref, scale)
    return _limit_cache[name]


def test_cpu_heavy_tail_leaves_the_robust_box():
    """The property of the input the clamped-outlier case rests on: the grid covers mean +- 3 sigma, and
    at least 2 % of this cloud lies outside that on some axis."""
    p, _ = _heavy_tail()
    out = (np.abs(p - p.mean(axis=0)) > 3.0 * p.std(axis=0)).any(axis=1)
    assert out.mean() >= 0.02, out.mean()


def test_cpu_any_partition_meets_the_large_softening_bound():
    """Limit 1 on the CPU: monopoles and second-order expansions of random partitions into 1, 7 and 300
    cells meet the bound on every row; with one source dropped, or counted twice, at least 99 % of the
    rows break it."""
    rs = np.random.RandomState(0)
    n = 3000
    p = rs.standard_t(2, size=(n, 3)) * 1e5 * AU
    m = rs.uniform(0.5, 2.0, n) * 1e-3 * SOLAR
    D = np.linalg.norm(p.max(axis=0) - p.min(axis=0))
    eps = EPS_OVER_D * D
    ref, scale = _direct(p, m, eps)
    assert (scale > 0).all()
    for ng in (1, 7, 300):
        lab = rs.randint(0, ng, n)
        for order in (1, 2):
            a = G * _partition_sum(p, m, lab, p, eps * eps, order)
            ratio = np.max(np.abs(a - ref) / scale)
            print("partition into %d, order %d: worst row %.3g of its scale (bound %.3g)" % (ng, order, ratio, TOL_LIMIT))
            assert ratio <= TOL_LIMIT, (ng, order, ratio)
    lab = rs.randint(0, 7, n)
    j = 5
    keep = np.arange(n) != j
    twice = np.append(np.arange(n), j)
    for what, idx in (("dropped", keep), ("doubled", twice)):
        for order in (1, 2):
            a = G * _partition_sum(p[idx], m[idx], lab[idx], p, eps * eps, order)
            broken = (np.abs(a - ref) > TOL_LIMIT * scale).any(axis=1)
            print("one source %s, order %d: %.4f of the rows break the bound" % (what, order, broken.mean()))
            assert broken.mean() >= 0.99, (what, order, broken.mean())


# =================================================================================================
# 2. a tight cluster seen from afar
# =================================================================================================
B_OVER_D = 0.03
NB, NT = 400, 600


def _c1(beta):
    return 0.75 / (1.0 - beta) ** 4


def _c2(beta):
    return 1.0 / (1.0 - beta) ** 5


def _cluster(d_factor=1.0, seed=41):
    """(points, mass, b, dist, c0): B = rows 0..NB-1, a bar inside the ball of radius b about c0; rows NB.. are
    zero-mass targets, half at d = b / 0.03 (* d_factor) from c0 and half at 2d; dist = their distance."""
    rs = np.random.RandomState(seed)
    b = 1e3 * AU
    d = d_factor * b / B_OVER_D
    c0 = np.array([0.7, -0.4, 0.2]) * d
    q = np.stack([rs.uniform(-1.0, 1.0, NB), 0.05 * rs.normal(size=NB), 0.05 * rs.normal(size=NB)], axis=1)
    q /= np.maximum(1.0, np.linalg.norm(q, axis=1) / 0.999)[:, None]
    u = rs.normal(size=(NT, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    dist = np.where(np.arange(NT) < NT // 2, d, 2.0 * d)
    p = np.vstack([c0 + b * q, c0 + dist[:, None] * u])
    m = np.append(rs.uniform(0.5, 2.0, NB) * 1e-3 * SOLAR, np.zeros(NT))
    assert np.linalg.norm(p[:NB] - c0, axis=1).max() <= b
    return np.ascontiguousarray(p), m, b, dist, c0


def _cluster_bounds(m, b, dist, eps):
    """(order-1 bound, order-2 bound) per target row, on the norm of the row's error"""
    M = m[:NB].sum()
    s = np.sqrt(dist ** 2 + eps ** 2)
    beta = b / dist
    return (_c1(beta) * G * M * (2 * b) ** 2 / s ** 4, _c2(beta) * G * M * (2 * b) ** 3 / s ** 5)


def test_cpu_multipole_remainder_bounds():
    """Limit 2 on the CPU, at eps/d = 0 and 0.5: over B as one cell, a random split into 8, the 8 octants
    about c0 (the cut a grid makes) and a split by a plane near one end, order 1 meets the C_1 bound and
    order 2 the C_2 bound on every target.  For B as one cell and for the random split (every part as long
    as B; a cut across the bar leaves shorter pieces with smaller errors of either order) order 1 misses
    the ORDER-2 bound on at least half the targets, and so does, on some target, the second-order term
    with 7.5 -> 6, with 1.5 -> 0 (at eps/d = 0.5: the trace part cancels at eps = 0) or with 3 -> -3."""
    p, m, b, dist, c0 = _cluster()
    pb, mb, xt = p[:NB], m[:NB], p[NB:]
    rs = np.random.RandomState(43)
    oct_lab = ((pb > c0) * np.array([1, 2, 4])).sum(axis=1)
    end_lab = (pb[:, 0] > c0[0] + 0.6 * b).astype(int)
    parts = {"one": np.zeros(NB, int), "random8": rs.randint(0, 8, NB), "octants": oct_lab, "end": end_lab}
    d = dist.min()
    for e_over_d in (0.0, 0.5):
        eps = e_over_d * d
        ref, scale = _direct(p, m, eps)
        ref, slack = ref[NB:], 1e-12 * np.linalg.norm(scale[NB:], axis=1)
        bound1, bound2 = _cluster_bounds(m, b, dist, eps)
        for name, lab in parts.items():
            e1 = np.linalg.norm(G * _partition_sum(pb, mb, lab, xt, eps * eps, 1) - ref, axis=1)
            e2 = np.linalg.norm(G * _partition_sum(pb, mb, lab, xt, eps * eps, 2) - ref, axis=1)
            print("eps/d %.1f, %-8s: order 1 up to %.3f of its bound, order 2 up to %.3f; median order 1 / order-2 bound %.2f"
                  % (e_over_d, name, (e1 / bound1).max(), (e2 / bound2).max(), np.median(e1 / bound2)))
            assert (e1 <= bound1 + slack).all(), (e_over_d, name)
            assert (e2 <= bound2 + slack).all(), (e_over_d, name)
            if name not in ("one", "random8"):
                continue
            assert (e1 > bound2 + slack).mean() >= 0.5, (e_over_d, name)
            mutants = [(6.0, 1.5, 3.0), (7.5, 1.5, -3.0)] + ([(7.5, 0.0, 3.0)] if e_over_d > 0 else [])
            for coef in mutants:
                em = np.linalg.norm(G * _partition_sum(pb, mb, lab, xt, eps * eps, 2, coef) - ref, axis=1)
                print("    coefficients %s: up to %.2f of the order-2 bound, %.2f of the rows beyond it"
                      % (coef, (em / bound2).max(), (em > bound2 + slack).mean()))
                assert (em > bound2 + slack).any(), (e_over_d, name, coef)


# =================================================================================================
# GPU
# =================================================================================================
@pytest.fixture(scope="module")
def tree_ctx():
    """tree_ctx(per_thread) -> a context of that walk.  SPHX_GRAV_KERNEL is read when a context is made."""
    from sph_code_amd import _lib
    made = {}

    def get(per_thread):
        if per_thread not in made:
            mp = pytest.MonkeyPatch()
            try:
                if per_thread:
                    mp.setenv("SPHX_GRAV_KERNEL", "0")
                else:
                    mp.delenv("SPHX_GRAV_KERNEL", raising=False)
                made[per_thread] = _lib.Context()
            finally:
                mp.undo()
        return made[per_thread]

    yield get
    for c in made.values():
        c.close()


def _tree(c, p, m, eps, ws, order, k_cells):
    from sph_code_amd import _lib
    dp = lambda a: a.ctypes.data_as(_lib.c_double_p)
    n = len(m)
    out = np.full((n, 3), np.nan)
    c.check(c.lib.sphx_set_gravity_order(c.h, order))
    c.check(c.lib.sphx_gravity_tree(c.h, n, dp(m), dp(p), None, float(eps), G, ws, k_cells, dp(out)))
    return out


KERNELS = (("wave", False), ("per-thread", True))
LIMIT_COMBOS = list(itertools.product((1, 2), (1, 2, 3, 4), (40, 1)))          # order, ws, k_cells


def _limit_failures(tree_ctx, p, m, eps, ref, scale, back=None):
    bad = []
    for kname, per_thread in KERNELS:
        c = tree_ctx(per_thread)
        for order, ws, kc in LIMIT_COMBOS:
            got = _tree(c, p, m, eps, ws, order, kc)
            if back is not None:
                got = got[back]
            miss = ~(np.abs(got - ref) <= TOL_LIMIT * scale)              # (a NaN misses)
            if miss.any():
                with np.errstate(all="ignore"):
                    worst = np.nanmax(np.where(scale > 0, np.abs(got - ref) / scale, 0.0))
                bad.append((kname, "order %d" % order, "ws %d" % ws, "k_cells %d" % kc,
                            "%d rows" % miss.any(axis=1).sum(), "first %d" % np.flatnonzero(miss.any(axis=1))[0],
                            "worst %.3g of its scale" % worst, "NaN" if np.isnan(got).any() else ""))
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(LIMIT_CASES))
def test_gpu_tree_counts_every_source_once(case, tree_ctx):
    """Limit 1 on both kernels, order 1 and 2, ws 1..4, coarse (k_cells 40) and fine (1) grids: every row
    within (4 (D/eps)^2 + 1e-12) of its scale of the oracle's direct sum, at eps = 1e6 D.
    gauss_5003_shift_20 / _27: the N = 5003 cloud 2^20 and 2^27 cloud sizes from the origin, the bound unchanged.  These
    hold only because the cells' centres of mass and the target - centre differences are formed about a point inside the
    cloud: on absolute coordinates a row inherits ulp(offset) / D instead of the round-off of the differences (worst
    |tree - direct| / scale against the bound 5e-12: 1.4e-14 at the origin, 5.0e-10 at 2^20, 1.2e-7 at 2^27)."""
    p, m, eps, ref, scale = _limit_case(case)
    bad = _limit_failures(tree_ctx, p, m, eps, ref, scale)
    assert not bad, bad


@pytest.mark.gpu
def test_gpu_tree_counts_every_source_once_permuted(tree_ctx):
    """The clamped-outlier cloud handed over in another order, the result put back: the same rows, the same
    bound (the grid's permutation and the output map)."""
    p, m, eps, ref, scale = _limit_case("heavy_tail")
    perm = np.random.RandomState(7).permutation(len(m))
    back = np.empty_like(perm)
    back[perm] = np.arange(len(m))
    bad = _limit_failures(tree_ctx, np.ascontiguousarray(p[perm]), np.ascontiguousarray(m[perm]), eps, ref, scale, back)
    assert not bad, bad


@pytest.mark.gpu
def test_gpu_tree_two_bodies_unsoftened(tree_ctx):
    """Two bodies at eps = 0: whatever the grid, each is either in the other's near field or alone in every
    cell that stands for it, and a cell of one particle IS that particle (no second moments, centre = the
    particle up to rounding) - so the tree gives the pair force, in both orders.  The masses are powers of
    two, which puts a lone particle's cell centre exactly on the particle."""
    p = np.array([[1.0e16, -2.0e16, 0.5e16], [-3.1e16, 1.7e16, 2.3e16]])
    m = np.array([2.0 ** 100, 2.0 ** 102])
    ref, scale = _direct(p, m, 0.0)
    bad = []
    for kname, per_thread in KERNELS:
        c = tree_ctx(per_thread)
        for order, ws, kc in LIMIT_COMBOS:
            got = _tree(c, p, m, 0.0, ws, order, kc)
            if not (np.abs(got - ref) <= 1e-12 * scale).all():
                bad.append((kname, order, ws, kc, got.tolist()))
    assert not bad, bad


N_FILL = 59000


@pytest.mark.gpu
@pytest.mark.parametrize("e_over_d", [0.0, 0.5])
def test_gpu_tree_multipole_terms(e_over_d, tree_ctx):
    """Limit 2 on both kernels at ws 1 and 2, k_cells = 1: order 1 within the C_1 bound and order 2 within
    the C_2 bound on every target row; order 1 beyond the order-2 bound on at least half of them.

    The rows prove something only if B is not in a target's near field (there the sum is direct): every
    target must be farther from B than 2 * cell_size * (2 ws + 2) * sqrt(3), cell_size read back from the
    library.  The grid's cell edge is a fixed fraction of the cloud's extent at a given particle count
    (about 0.15 d for these 1000 particles, and never under 0.12 d: the grid is capped at 32 n + 1024 cells),
    so a larger d alone cannot meet that; N_FILL more zero-mass particles on the same two shells bring the
    cell edge to about 0.035 d.  They feel B and weigh nothing, as the 600 targets do."""
    p, m, b, dist, c0 = _cluster()
    d = dist.min()
    eps = e_over_d * d
    ref, scale = _direct(p, m, eps)
    ref, slack = ref[NB:], 1e-12 * np.linalg.norm(scale[NB:], axis=1)
    bound1, bound2 = _cluster_bounds(m, b, dist, eps)
    rs = np.random.RandomState(47)
    u = rs.normal(size=(N_FILL, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    fill = c0 + (d * np.where(np.arange(N_FILL) % 2 == 0, 1.0, 2.0))[:, None] * u
    pf = np.ascontiguousarray(np.vstack([p, fill]))
    mf = np.append(m, np.zeros(N_FILL))
    bad = []
    for kname, per_thread in KERNELS:
        c = tree_ctx(per_thread)
        for ws in (1, 2):
            err = {}
            for order in (1, 2):
                got = _tree(c, pf, mf, eps, ws, order, 1)
                assert np.isfinite(got).all(), (kname, ws, order)
                cell = c.stats()["cell_size"]
                assert d - b > 2.0 * cell * (2 * ws + 2) * np.sqrt(3.0), (kname, ws, cell / d)
                err[order] = np.linalg.norm(got[NB:NB + NT] - ref, axis=1)
            print("eps/d %.1f %s ws %d (cell %.4f d): order 1 up to %.3f of its bound, order 2 up to %.3f; "
                  "order 1 beyond the order-2 bound on %.2f of the rows"
                  % (e_over_d, kname, ws, cell / d, (err[1] / bound1).max(), (err[2] / bound2).max(),
                     (err[1] > bound2 + slack).mean()))
            if not (err[1] <= bound1 + slack).all():
                bad.append((kname, ws, "order 1", (err[1] / bound1).max()))
            if not (err[2] <= bound2 + slack).all():
                bad.append((kname, ws, "order 2", (err[2] / bound2).max()))
            if not (err[1] > bound2 + slack).mean() >= 0.5:
                bad.append((kname, ws, "order 1 within the order-2 bound", (err[1] > bound2 + slack).mean()))
    assert not bad, bad
