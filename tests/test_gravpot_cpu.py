"""The gravitational potential (include/sphx.h: sphx_gravity_direct_pot, sphx_gravity_tree_pot) on the CPU: the NumPy
restatement tests/gravpot_oracle.py against closed forms and against the oracle's acceleration, and the two bounds the
GPU tests (test_gpu_gravpot.py) hold the tree's potential to, proven here on NumPy restatements of a cell's expansion
over arbitrary partitions, together with the mutations that must break them.

Throughout f(r) = 1 / sqrt(|r|^2 + eps^2), s^2 = |r|^2 + eps^2, and - as tests/test_gravity_tree_rows.py shows from the
generating function of the Legendre polynomials - the k-th derivative of f, a symmetric k-linear form, has norm
<= k! / s^(k+1).

0. Central difference.  phi(x) = -G sum m_j f(x_j - x), a = -grad phi.  For a zero-mass probe moved by +-h along x,
       (phi(x + h) - phi(x - h)) / (2h) = d phi / dx + h^2 / 6 * phi'''(xi),      |xi - x| <= h,
   and the third derivative of one term is at most G m_j 3! / s_j(xi)^4 with s_j(xi) >= s_j - h (|grad s| <= 1):
       |cd + a_x| <= h^2 sum_j G m_j / (s_j - h)^4                                   (truncation)
   Round-off: a computed phi differs from the exact sum of its terms by at most (n + 8) u sum_j |term_j|, u = 2^-53 (n
   for the summation in any order, 8 for the operations of a term: the difference of exact inputs, three squares and
   their sum, eps^2, sqrt, the division); the difference of the two adds u |phi|, and the quotient by the exactly
   representable 2h nothing more that matters: (2 (n + 8) + 1) u sum_j |term_j| / (2h).  The oracle's own row carries
   (n + 8) u sum_j |a-term_j|, which its return_abs gives.  Probes and h are multiples of 2^20 m, so x +- h is exact.

1. Large softening (eps = 1e6 D, D the diagonal of the true bounding box).  With g(u) = (u + eps^2)^(-1/2), u = |d|^2:
   g(u) = 1 / eps - u / (2 eps^3) + R, |R| <= 3/8 u^2 / eps^5 (g'' <= 3/4 eps^-5).  Every source and every centre of
   mass lies in the box, so u <= D^2.  One cell (M, c; delta = x_j - c, S = sum m delta delta^T, tr S <= M D^2), target
   outside it, d_j = x_j - x, r = c - x:
     order 1   sum m g(|d_j|^2) - M g(|r|^2) = -(sum m |d_j|^2 - M |r|^2) / (2 eps^3) + R' = -tr S / (2 eps^3) + R',
               the parallel-axis term, |R'| <= 3/4 M D^4 / eps^5: at most (M / eps) [1/2 (D/eps)^2 + 3/4 (D/eps)^4];
     order 2   adds 3/2 (r.S.r) / s^5 - 1/2 tr S / s^3: the second removes the parallel-axis term up to
               1/2 tr S |1/eps^3 - 1/s^3| <= 3/4 M D^4 / eps^5, the first is at most 3/2 M D^4 / eps^5:
               at most 3 (M / eps) (D/eps)^4.
   A row's scale is sum_{j != i} m_j / s_ij >= (sum_{j != i} m_j / eps) / sqrt(1 + (D/eps)^2), and the cells of a
   partition that does not hold the target add up to at most sum_{j != i} m_j; the target's own cell is summed directly,
   row i left out by index.  So for ANY partition, of either order,
       |phi_tree_i - phi_direct_i| <= (c (D/eps)^2 + 1e-12) sum_j |term_ij|,        c = 1
   (1/2 from the parallel-axis term of order 1, the rest - a factor 2 - for the higher terms and sqrt(1 + (D/eps)^2);
   1e-12 is the round-off allowance of the acceleration's rows).  A source dropped or doubled moves a row by
   m_j / eps, about 1 / N of its scale, and so does the self term if it is let in: all three eight orders above the bound.

2. Multipole remainder.  The bar cluster B of test_gravity_tree_rows.py (mass M inside a ball of radius b about c0,
   targets at distance d and 2d).  Expand sum m f(r + delta) about a cell's centre of mass (sum m delta = 0):
     order 1 leaves  sum m int_0^1 (1 - t) D^2 f(r + t delta)[delta, delta] dt <= 1/2 * 2! / s_min^3 * sum m |delta|^2,
     order 2 leaves  at most 1/6 * 3! / s_min^4 * sum m |delta|^3,
   s_min >= (1 - b/d) s, sum m |delta|^2 <= M b^2 = M (2b)^2 / 4, sum m |delta|^3 <= M (2b)^3 / 4.  Hence
       |phi_tree - phi_direct| <= C'_p G M (2b)^(p+1) / s^(p+2),   C'_1 = 0.25 / (1 - b/d)^3,  C'_2 = 0.25 / (1 - b/d)^4
   for any sub-partition of B.  B is a bar, so that the order-1 error (1/2 |3 (r.S.r) / s^5 - tr S / s^3|, with
   S ~ M b^2 / 3 along the axis: 0.042 |3 cos^2 - 1| G M (2b)^2 / s^3 at eps = 0) stands clear of the ORDER-2 bound
   (0.017 of the same unit at d, half that at 2d) on most targets, and a wrong coefficient of the second-order term too."""
import numpy as np

import gravpot_oracle as gpo
from test_gravity_tree_rows import (AU, B_OVER_D, EPS_OVER_D, G, NB, SOLAR, _cluster, _direct, _gauss)

C_LIMIT = 1.0
TOL_LIMIT_POT = C_LIMIT / EPS_OVER_D ** 2 + 1e-12
POT_COEF = (1.5, 0.5)
U53 = 2.0 ** -53


def c1_pot(beta):
    return 0.25 / (1.0 - beta) ** 3


def c2_pot(beta):
    return 0.25 / (1.0 - beta) ** 4


def cluster_pot_bounds(m, b, dist, eps):
    """(order-1 bound, order-2 bound) on |phi_tree - phi_direct| per target row of the bar cluster"""
    M = m[:NB].sum()
    s = np.sqrt(dist ** 2 + eps ** 2)
    beta = b / dist
    return c1_pot(beta) * G * M * (2 * b) ** 2 / s ** 3, c2_pot(beta) * G * M * (2 * b) ** 3 / s ** 4


# =================================================================================================
# NumPy restatement of a cell's expansion of the potential
# =================================================================================================
def _expand_pot(ps, ms, xt, e2, order, coef=POT_COEF):
    """-phi / G at the targets xt (t,3) of the sources (ps, ms) taken as ONE cell (the header's phi_cell)."""
    M = ms.sum()
    c = (ms[:, None] * ps).sum(axis=0) / M
    r = c - xt
    s = np.sqrt((r * r).sum(axis=1) + e2)
    v = M / s
    if order == 2:
        dl = ps - c
        S = (ms[:, None, None] * dl[:, :, None] * dl[:, None, :]).sum(axis=0)
        rSr = (r * (r @ S)).sum(axis=1)
        v = v + coef[0] * rSr / s ** 5 - coef[1] * np.trace(S) / s ** 3
    return v


def _partition_pot(ps, ms, lab, xt, e2, order, coef=POT_COEF):
    """phi / G at targets that are none of the sources: every cell of the partition expanded"""
    v = np.zeros(len(xt))
    for g in np.unique(lab):
        sel = lab == g
        if ms[sel].sum() > 0.0:
            v += _expand_pot(ps[sel], ms[sel], xt, e2, order, coef)
    return -v


def _partition_pot_rows(p, m, lab, e2, order, self_term=False):
    """phi / G of every row of the cloud as a tree forms it: the cells that do not hold the row expanded, the row's own
    cell summed directly with the row left out by index (self_term: let in)."""
    n = len(m)
    v = np.zeros(n)
    idx = np.arange(n)
    for g in np.unique(lab):
        sel = lab == g
        if not ms_positive(m[sel]):
            continue
        out = ~sel
        if out.any():
            v[out] += _expand_pot(p[sel], m[sel], p[out], e2, order)
        own = idx[sel]
        near, _ = gpo.potential_at(p[own], p[own], m[own], np.sqrt(e2), G=1.0,
                                   exclude=None if self_term else np.arange(len(own)))
        v[own] -= near
    return -v


def ms_positive(ms):
    return ms.sum() > 0.0


# =================================================================================================
# the restatement itself
# =================================================================================================
def test_two_bodies_closed_form():
    p = np.array([[1.0e16, -2.0e16, 0.5e16], [-3.1e16, 1.7e16, 2.3e16]])
    m = np.array([3.0e30, 5.0e29])
    r2 = float(((p[1] - p[0]) ** 2).sum())
    for eps in (0.0, 1.0e16, 7.0e17):
        phi, scale = gpo.potential_direct(p, m, eps, G=G)
        want = -G * m[::-1] / np.sqrt(r2 + eps * eps)
        assert np.all(np.abs(phi - want) <= 8 * U53 * np.abs(want)), (eps, phi, want)
        assert np.all(np.abs(scale + want) <= 8 * U53 * np.abs(want))
        U = gpo.total(m, phi)
        assert abs(U + G * m[0] * m[1] / np.sqrt(r2 + eps * eps)) <= 16 * U53 * abs(U)
    # a lone body, and two on one point: nothing at eps = 0, -G m / eps otherwise; the self term never enters
    assert gpo.potential_direct(p[:1], m[:1], 1.0e16, G=G)[0][0] == 0.0
    twin = np.vstack([p[0], p[0]])
    assert np.all(gpo.potential_direct(twin, m, 0.0, G=G)[0] == 0.0)
    got = gpo.potential_direct(twin, m, 2.0e15, G=G)[0]
    assert np.all(np.abs(got + G * m[::-1] / 2.0e15) <= 4 * U53 * np.abs(got))


def test_uniform_shell_closed_form():
    """The twelve vertices of an icosahedron, equal masses, radius R, eps = 0.  From the centre every source is at R:
    phi = -G M / R to round-off.  From outside at distance d: phi = -G M sum_l R^l / d^(l+1) <P_l>, and the moments of
    order 1..5 of a set with the icosahedron's symmetry vanish (its group has no invariant below order 6):
    |phi + G M / d| <= G M / d * (R/d)^6 / (1 - R/d)."""
    t = (1.0 + np.sqrt(5.0)) / 2.0
    v = np.array([[0, s1, s2 * t] for s1 in (-1, 1) for s2 in (-1, 1)], dtype=np.float64)
    v = np.vstack([v, v[:, [2, 0, 1]], v[:, [1, 2, 0]]])
    R = 3.0e15
    v *= R / np.linalg.norm(v, axis=1)[:, None]
    m = np.full(12, 2.0e29)
    M = m.sum()
    centre, _ = gpo.potential_at(np.zeros((1, 3)), v, m, 0.0, G=G)
    assert abs(centre[0] + G * M / R) <= 32 * U53 * G * M / R
    rs = np.random.RandomState(3)
    u = rs.normal(size=(40, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    for ratio in (4.0, 8.0):
        d = ratio * R
        phi, _ = gpo.potential_at(d * u, v, m, 0.0, G=G)
        bound = G * M / d * (1.0 / ratio) ** 6 / (1.0 - 1.0 / ratio)
        err = np.abs(phi + G * M / d)
        print("shell from %.0f R: worst %.3g of -GM/d, bound %.3g" % (ratio, err.max() / (G * M / d), bound / (G * M / d)))
        assert np.all(err <= bound + 32 * U53 * G * M / d)
        assert err.max() > 1e-3 * bound            # (the l = 6 term is there: the check is not vacuous)


def test_central_difference_reproduces_the_oracles_acceleration():
    """Bound 0 of the module docstring on 48 zero-mass probes in a cloud of 257, eps = 0 and eps = 0.05 of the cloud."""
    from oracle import sph_oracle as orc
    ps, ms = _gauss(257, 357)
    rs = np.random.RandomState(358)
    q = 2.0 ** 20
    probes = np.round(rs.normal(size=(48, 3)) * 1e5 * AU / q) * q
    h = 2.0 ** 40
    n = len(ms)
    p_all = np.vstack([ps, probes])
    m_all = np.append(ms, np.zeros(len(probes)))
    for eps in (0.0, 0.05 * 1e5 * AU):
        acc, acc_abs = orc.gravity_direct(p_all, m_all, eps, G=G, return_abs=True)
        for ax in range(3):
            step = np.zeros(3)
            step[ax] = h
            assert np.all((probes + step) - probes == step) and np.all(probes - (probes - step) == step)
            php, sp = gpo.potential_at(probes + step, ps, ms, eps, G=G)
            phm, sm = gpo.potential_at(probes - step, ps, ms, eps, G=G)
            cd = (php - phm) / (2.0 * h)
            sj = np.sqrt(((ps[None, :, :] - probes[:, None, :]) ** 2).sum(axis=2) + eps * eps)
            assert (sj > 2.0 * h).all()
            trunc = h * h * G * (ms[None, :] / (sj - h) ** 4).sum(axis=1)
            rnd = (2 * (n + 8) + 1) * U53 * np.maximum(sp, sm) / (2.0 * h) + (n + 8) * U53 * acc_abs[n:, ax]
            err = np.abs(cd + acc[n:, ax])
            print("eps %.2g axis %d: worst error %.3g of its bound (truncation share %.2f)"
                  % (eps, ax, (err / (trunc + rnd)).max(), np.median(trunc / (trunc + rnd))))
            assert np.all(err <= trunc + rnd), (eps, ax)
            # the bound says something: it is far below the acceleration itself
            assert np.median((trunc + rnd) / np.abs(acc[n:, ax])) < 1e-4


# =================================================================================================
# 1. the large-softening limit
# =================================================================================================
def test_any_partition_meets_the_large_softening_bound():
    """Random partitions into 1, 7 and 300 cells, order 1 and 2, meet bound 1 on every row; order 1's error is the
    parallel-axis term and order 2 removes it; one source dropped, one doubled, or the self term let in, and at least
    99 % of the rows break the bound."""
    rs = np.random.RandomState(0)
    n = 3000
    p = rs.standard_t(2, size=(n, 3)) * 1e5 * AU
    m = rs.uniform(0.5, 2.0, n) * 1e-3 * SOLAR
    D = np.linalg.norm(p.max(axis=0) - p.min(axis=0))
    eps = EPS_OVER_D * D
    ref, scale = gpo.potential_direct(p, m, eps, G=G)
    assert (scale > 0).all()
    for ng in (1, 7, 300):
        lab = rs.randint(0, ng, n)
        worst = {}
        for order in (1, 2):
            got = G * _partition_pot_rows(p, m, lab, eps * eps, order)
            worst[order] = np.max(np.abs(got - ref) / scale)
            print("partition into %d, order %d: worst row %.3g of its scale (bound %.3g)" % (ng, order, worst[order], TOL_LIMIT_POT))
            assert worst[order] <= TOL_LIMIT_POT, (ng, order, worst[order])
    # what order 1 leaves IS the parallel-axis term -G tr S / (2 eps^3), up to 3/4 G M D^4 / eps^5, and order 2 leaves at
    # most 3 G M D^4 / eps^5: one cell over everything, seen by zero-mass probes, at eps = 100 D where (D/eps)^2 = 1e-4
    # of a row stands clear of the round-off
    probes = p[:50] * 0.9
    eps_pa = 100.0 * D
    d1, s1 = gpo.potential_at(probes, p, m, eps_pa, G=G)
    e1 = G * _partition_pot(p, m, np.zeros(n, int), probes, eps_pa ** 2, 1) - d1
    e2 = G * _partition_pot(p, m, np.zeros(n, int), probes, eps_pa ** 2, 2) - d1
    c = (m[:, None] * p).sum(axis=0) / m.sum()
    axis_term = 0.5 * G * (m * ((p - c) ** 2).sum(axis=1)).sum() / eps_pa ** 3
    fourth = G * m.sum() * D ** 4 / eps_pa ** 5
    slack = 2 * (n + 8) * U53 * s1
    print("eps = 100 D: order 1 leaves %.6g .. %.6g, the parallel-axis term is %.6g; order 2 leaves up to %.3g (G M D^4 / eps^5 = %.3g)"
          % (e1.min(), e1.max(), -axis_term, np.abs(e2).max(), fourth))
    assert axis_term > 100 * slack.max()
    assert np.all(np.abs(e1 + axis_term) <= 0.75 * fourth + slack)
    assert np.all(np.abs(e2) <= 3.0 * fourth + slack)
    lab = rs.randint(0, 7, n)
    j = 5
    keep = np.arange(n) != j
    twice = np.append(np.arange(n), j)
    for what, idx in (("dropped", keep), ("doubled", twice)):
        for order in (1, 2):
            # the rows of the changed cloud against the reference rows of the same particles
            got = G * _partition_pot_rows(p[idx], m[idx], lab[idx], eps * eps, order)
            rows = np.flatnonzero(idx) if what == "dropped" else np.arange(n)
            broken = np.abs(got[:len(rows)] - ref[rows]) > TOL_LIMIT_POT * scale[rows]
            print("one source %s, order %d: %.4f of the rows break the bound" % (what, order, broken.mean()))
            assert broken.mean() >= 0.99, (what, order, broken.mean())
    for order in (1, 2):
        got = G * _partition_pot_rows(p, m, lab, eps * eps, order, self_term=True)
        broken = np.abs(got - ref) > TOL_LIMIT_POT * scale
        print("self term let in, order %d: %.4f of the rows break the bound" % (order, broken.mean()))
        assert broken.mean() >= 0.99, (order, broken.mean())


# =================================================================================================
# 2. the multipole remainder
# =================================================================================================
MUTANTS = [(1.0, 0.5), (0.0, 0.5), (-0.5, 0.5), (1.5, 1.0), (1.5, 0.0), (1.5, -0.5)]


def test_multipole_remainder_bounds():
    """Limit 2 at eps/d = 0 and 0.5, targets at d and 2d: over B as one cell, a random split into 8, the octants about c0
    and a cut near one end, order 1 meets the C'_1 bound and order 2 the C'_2 bound on every target.  For B as one cell
    and the random split, order 1 misses the ORDER-2 bound on at least half the targets, and so does - on some target -
    the second-order term with 1.5 or 0.5 changed to 1, 0 or -0.5."""
    assert abs(B_OVER_D - 0.03) < 1e-15
    p, m, b, dist, c0 = _cluster()
    pb, mb, xt = p[:NB], m[:NB], p[NB:]
    assert set(np.round(dist / dist.min()).astype(int)) == {1, 2}
    rs = np.random.RandomState(43)
    oct_lab = ((pb > c0) * np.array([1, 2, 4])).sum(axis=1)
    end_lab = (pb[:, 0] > c0[0] + 0.6 * b).astype(int)
    parts = {"one": np.zeros(NB, int), "random8": rs.randint(0, 8, NB), "octants": oct_lab, "end": end_lab}
    d = dist.min()
    for e_over_d in (0.0, 0.5):
        eps = e_over_d * d
        ref, scale = gpo.potential_at(xt, pb, mb, eps, G=G)
        slack = 1e-12 * scale
        bound1, bound2 = cluster_pot_bounds(m, b, dist, eps)
        for name, lab in parts.items():
            e1 = np.abs(G * _partition_pot(pb, mb, lab, xt, eps * eps, 1) - ref)
            e2 = np.abs(G * _partition_pot(pb, mb, lab, xt, eps * eps, 2) - ref)
            print("eps/d %.1f, %-8s: order 1 up to %.3f of its bound, order 2 up to %.3f; order 1 beyond the order-2 bound on %.2f"
                  % (e_over_d, name, (e1 / bound1).max(), (e2 / bound2).max(), (e1 > bound2 + slack).mean()))
            assert (e1 <= bound1 + slack).all(), (e_over_d, name)
            assert (e2 <= bound2 + slack).all(), (e_over_d, name)
            if name not in ("one", "random8"):
                continue
            assert (e1 > bound2 + slack).mean() >= 0.5, (e_over_d, name)
            for coef in MUTANTS:
                em = np.abs(G * _partition_pot(pb, mb, lab, xt, eps * eps, 2, coef) - ref)
                print("    coefficients %s: up to %.2f of the order-2 bound, %.2f of the rows beyond it"
                      % (coef, (em / bound2).max(), (em > bound2 + slack).mean()))
                assert (em > bound2 + slack).any(), (e_over_d, name, coef)


def test_the_cell_term_is_the_potential_of_the_acceleration_term():
    """Minus the gradient in x of the header's phi_cell is the acceleration term of test_gravity_tree_rows._expand (7.5,
    1.5, 3): central difference of the restatement above, bound as in 0. with the fourth derivative of the cell's
    expansion - here simply 1e-6 of the acceleration at h = 2^-12 of the distance (the h^2 term is ~6e-8 of it)."""
    from test_gravity_tree_rows import _expand
    p, m, b, dist, c0 = _cluster()
    pb, mb, xt = p[:NB], m[:NB], p[NB:NB + 40]
    for e_over_d in (0.0, 0.5):
        e2 = (e_over_d * dist.min()) ** 2
        a = _expand(pb, mb, xt, e2, 2)
        h = dist.min() * 2.0 ** -12
        for ax in range(3):
            step = np.zeros(3)
            step[ax] = h
            cd = (-_expand_pot(pb, mb, xt + step, e2, 2) + _expand_pot(pb, mb, xt - step, e2, 2)) / (2.0 * h)
            assert np.all(np.abs(-cd - a[:, ax]) <= 1e-6 * np.linalg.norm(a, axis=1)), (e_over_d, ax)
