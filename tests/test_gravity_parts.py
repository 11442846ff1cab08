"""Gravity between parts (sphx_gravity_tree_parts: the export rule, the export kernels, the remote sum), held to the
row-by-row bounds of test_gravity_tree_rows.py, which were derived there for ANY partition of the sources into cells.

The export rule.  A part exports its mass to a peer as a flat list decided against Q, the peer's bounding box:
box(c) is the cell's box (face cells reach out to the part's true bounding box), accept(c) means
dist(box(c), Q) >= ws * longest edge of box(c), a cell travels as one record iff it is the first accepted cell on the
way down from the top cell, and the particles of level-1 cells never accepted travel as particles.  The CPU part
restates the rule in NumPy on a pyramid of its own and proves that the records partition the particles - through the
large-softening bound, which a dropped or doubled record breaks on (nearly) every row.  The GPU part holds the library
to the same bounds through compat.grav_force_tree_parts, which runs every new kernel on one context."""
import numpy as np
import pytest

from test_gravity_tree_rows import (AU, SOLAR, G, EPS_OVER_D, TOL_LIMIT, NB, _expand, _direct, _cluster, _c1, _c2)


# =================================================================================================
# the rule in NumPy
# =================================================================================================
class ModelPyramid:
    """A pyramid over the points p: fine cells of edge `cell` on the box mean +- 3 sigma (cut to the true box), outliers
    clamped into the face cells; level l has cells of 2^l fine cells a side; the top level is one cell."""

    def __init__(self, p, cell_frac=0.08):
        self.p = p
        self.tlo, self.thi = p.min(axis=0), p.max(axis=0)
        mean, sd = p.mean(axis=0), p.std(axis=0)
        self.glo = np.maximum(self.tlo, mean - 3.0 * sd)
        ghi = np.minimum(self.thi, mean + 3.0 * sd)
        ext = max((ghi - self.glo).max(), 1.0)
        self.cell = cell_frac * ext
        self.nf = np.floor((ghi - self.glo) / self.cell).astype(int) + 1
        self.fine = np.clip(np.floor((p - self.glo) / self.cell).astype(int), 0, self.nf - 1)
        self.nlev = 1
        while ((self.nf + (1 << self.nlev) - 1) >> self.nlev).max() > 1:
            self.nlev += 1
        self.lo = np.minimum(self.glo, self.tlo)
        self.hi = np.maximum(self.glo + self.nf * self.cell, self.thi)

    def box(self, l, idx):
        f0, f1 = idx << l, (idx + 1) << l
        lo = np.where(idx == 0, self.lo, self.glo + f0 * self.cell)
        hi = np.where(f1 >= self.nf, self.hi, self.glo + f1 * self.cell)
        return lo, hi

    def accept(self, l, idx, qlo, qhi, ws):
        lo, hi = self.box(l, idx)
        gap = np.maximum(0.0, np.maximum(qlo - hi, lo - qhi))
        return ws > 0 and np.sqrt((gap * gap).sum()) >= ws * (hi - lo).max()

    def export(self, qlo, qhi, ws):
        """-> list of member-index arrays: one per multipole record, then one per particle record."""
        cells, parts = [], []
        for l in range(self.nlev, 0, -1):
            keys = np.unique(self.fine >> l, axis=0)
            for idx in keys:
                first = 0
                for L in range(self.nlev, l - 1, -1):
                    if self.accept(L, idx >> (L - l), qlo, qhi, ws):
                        first = L
                        break
                members = np.flatnonzero(((self.fine >> l) == idx).all(axis=1))
                if first == l:
                    cells.append(members)
                elif first == 0 and l == 1:
                    parts.extend(np.array([j]) for j in members)
        return cells, parts


def _fill_box(qlo, qhi, n, seed):
    """n points inside [qlo, qhi] whose bounding box is exactly that box"""
    rs = np.random.RandomState(seed)
    q = qlo + (qhi - qlo) * rs.uniform(size=(n, 3))
    if n >= 2:
        q[0], q[1] = qlo, qhi
    return q


def _exporter(seed, heavy):
    rs = np.random.RandomState(seed)
    n = 600
    p = (rs.standard_t(2, size=(n, 3)) if heavy else rs.normal(size=(n, 3))) * 1e5 * AU
    return p, rs.uniform(0.5, 2.0, n) * 1e-3 * SOLAR


R = 1e5 * AU
BOX_CASES = {
    # name: (heavy-tailed exporter, Q lo, Q hi in units of the exporter's sigma)
    "far": (False, (40.0, -3.0, -3.0), (46.0, 3.0, 3.0)),
    "touching": (False, None, None),                    # Q starts exactly where the exporter's true box ends
    "overlapping": (False, (0.5, -1.0, -1.0), (6.0, 4.0, 2.0)),
    "containing": (False, (-9.0, -9.0, -9.0), (9.0, 9.0, 9.0)),
    "point": (False, (7.0, 5.0, -6.0), (7.0, 5.0, -6.0)),
    "outliers": (True, (12.0, -2.0, -2.0), (18.0, 4.0, 4.0)),
}


def _box_case(name):
    heavy, lo, hi = BOX_CASES[name]
    p, m = _exporter(3, heavy)
    if lo is None:
        qlo = np.array([p[:, 0].max(), p[:, 1].min(), p[:, 2].min()])
        qhi = qlo + np.array([5.0, 4.0, 3.0]) * R
    else:
        qlo, qhi = np.array(lo) * R, np.array(hi) * R
    nq = 1 if name == "point" else 300
    q = _fill_box(qlo, qhi, nq, 9)
    mq = np.random.RandomState(10).uniform(0.5, 2.0, nq) * 1e-3 * SOLAR
    return p, m, q, mq, qlo, qhi


def _field_of_records(p, m, records, xt, e2, order):
    a = np.zeros_like(xt)
    for mem in records:
        if m[mem].sum() > 0.0:
            a += _expand(p[mem], m[mem], xt, e2, order)
    return a


@pytest.mark.parametrize("name", sorted(BOX_CASES))
@pytest.mark.parametrize("ws", [1, 2])
def test_cpu_export_rule_partitions_the_particles(name, ws):
    """The exported records hold every particle of the exporter exactly once, for a peer box that is far, touching,
    overlapping, containing the exporter, a point, and for an exporter with outliers beyond its grid; the field they
    give the peer's particles meets the large-softening bound on every row in both orders, and with one record dropped
    or doubled at least 99 % of the rows break it."""
    p, m, q, mq, qlo, qhi = _box_case(name)
    pyr = ModelPyramid(p)
    if name == "outliers":
        out = ((p < pyr.glo) | (p >= pyr.glo + pyr.nf * pyr.cell)).any(axis=1)
        assert out.mean() >= 0.02, out.mean()
    cells, parts = pyr.export(qlo, qhi, ws)
    records = cells + parts
    seen = np.concatenate(records)
    assert len(seen) == len(p) and (np.sort(seen) == np.arange(len(p))).all(), name
    if name == "far":
        assert len(cells) >= 1 and not parts
    if name == "containing":
        assert not cells and len(parts) == len(p)
    # every multipole record keeps its clearance: all its members lie ws edges of its box from Q
    allp = np.vstack([p, q]); allm = np.append(m, mq)
    D = np.linalg.norm(allp.max(axis=0) - allp.min(axis=0))
    eps = EPS_OVER_D * D
    ref, scale = _direct(allp, allm, eps)
    ref, scale = ref[len(p):], scale[len(p):]
    own = G * _field_of_records(q, mq, [np.array([j]) for j in range(len(q))], q, eps * eps, 1)
    for order in (1, 2):
        a = own + G * _field_of_records(p, m, records, q, eps * eps, order)
        ratio = np.max(np.abs(a - ref) / scale)
        print("%s ws %d order %d: %d cells, %d particles, worst row %.3g of its scale (bound %.3g)"
              % (name, ws, order, len(cells), len(parts), ratio, TOL_LIMIT))
        assert ratio <= TOL_LIMIT, (name, ws, order, ratio)
        j = len(records) // 2
        for what, recs in (("dropped", records[:j] + records[j + 1:]), ("doubled", records + [records[j]])):
            b = own + G * _field_of_records(p, m, recs, q, eps * eps, order)
            broken = (np.abs(b - ref) > TOL_LIMIT * scale).any(axis=1)
            assert broken.mean() >= 0.99, (name, ws, order, what, broken.mean())


def test_cpu_export_rule_never_accepts_at_ws_0():
    p, m, q, mq, qlo, qhi = _box_case("far")
    cells, parts = ModelPyramid(p).export(qlo, qhi, 0)
    assert not cells and len(parts) == len(p)


# =================================================================================================
# the bar cluster seen from two balls (the remote multipole term)
# =================================================================================================
NT_BALL = 600


def _bar_and_balls(direction=(0.7, -0.4, 0.2), seed=51):
    """(points, mass, b, dist, part_of): rows 0..NB-1 the bar cluster B of test_gravity_tree_rows._cluster (part 0), then
    600 zero-mass targets (part 1) in two balls of radius 3b centred d and 2d from B's centre, d = b / 0.03; dist =
    each target's own distance from B's centre."""
    p0, m0, b, _, c0 = _cluster()
    d = b / 0.03
    u = np.asarray(direction, dtype=np.float64)
    u /= np.linalg.norm(u)
    rs = np.random.RandomState(seed)
    v = rs.normal(size=(NT_BALL, 3))
    v *= (3.0 * b * rs.uniform(size=NT_BALL) ** (1.0 / 3.0) / np.linalg.norm(v, axis=1))[:, None]
    centre = c0 + np.where(np.arange(NT_BALL) < NT_BALL // 2, d, 2.0 * d)[:, None] * u
    t = centre + v
    p = np.ascontiguousarray(np.vstack([p0[:NB], t]))
    m = np.append(m0[:NB], np.zeros(NT_BALL))
    dist = np.linalg.norm(t - c0, axis=1)
    lab = np.append(np.zeros(NB, np.int32), np.ones(NT_BALL, np.int32))
    return p, m, b, dist, lab


def _bar_bounds(m, b, dist, eps):
    M = m[:NB].sum()
    s = np.sqrt(dist ** 2 + eps ** 2)
    beta = b / dist
    return _c1(beta) * G * M * (2 * b) ** 2 / s ** 4, _c2(beta) * G * M * (2 * b) ** 3 / s ** 5


def test_cpu_bar_as_one_cell_meets_its_bounds_from_the_balls():
    """What the GPU test of the remote term relies on: with B as ONE cell, seen from the two balls in six directions at
    eps/d = 0 and 0.5, order 1 stays within the C_1 bound and order 2 within the C_2 bound on every target, and order 1
    lies beyond the ORDER-2 bound on at least half of them."""
    dirs = [(0.7, -0.4, 0.2), (-0.7, 0.4, -0.2), (1, 0, 0), (0, -1, 0), (0, 0, 1), (0.3, 0.3, -0.9)]
    for u in dirs:
        p, m, b, dist, _ = _bar_and_balls(u)
        d = b / 0.03
        for e_over_d in (0.0, 0.5):
            eps = e_over_d * d
            ref, scale = _direct(p, m, eps)
            ref, slack = ref[NB:], 1e-12 * np.linalg.norm(scale[NB:], axis=1)
            bound1, bound2 = _bar_bounds(m, b, dist, eps)
            e1 = np.linalg.norm(G * _expand(p[:NB], m[:NB], p[NB:], eps * eps, 1) - ref, axis=1)
            e2 = np.linalg.norm(G * _expand(p[:NB], m[:NB], p[NB:], eps * eps, 2) - ref, axis=1)
            print("direction %s eps/d %.1f: order 1 up to %.3f of its bound, order 2 up to %.4f, order 1 beyond the "
                  "order-2 bound on %.2f of the rows" % (u, e_over_d, (e1 / bound1).max(), (e2 / bound2).max(),
                                                         (e1 > bound2 + slack).mean()))
            assert (e1 <= bound1 + slack).all() and (e2 <= bound2 + slack).all(), (u, e_over_d)
            assert (e1 > bound2 + slack).mean() >= 0.5, (u, e_over_d)


# =================================================================================================
# GPU
# =================================================================================================
def _gauss(n, seed):
    rs = np.random.RandomState(seed)
    return rs.normal(size=(n, 3)) * 1e5 * AU, rs.uniform(0.5, 2.0, n) * 1e-3 * SOLAR


def _heavy_tail(n=5003, seed=5):
    rs = np.random.RandomState(seed)
    return rs.standard_t(2, size=(n, 3)) * 1e5 * AU, rs.uniform(0.5, 2.0, n) * 1e-3 * SOLAR


def _zero_scattered():
    p, m = _gauss(3000, 23)
    m[np.random.RandomState(24).rand(3000) < 0.3] = 0.0
    return p, m


def _shifted(m_, n=5003):
    """the N = 5003 cloud 2^m_ cloud sizes from the origin, snapped to a lattice first so that the shift is exact"""
    p, m = _gauss(n, 100 + n)
    R0 = 2.0 ** np.ceil(np.log2(np.abs(p).max()))
    p = np.round(p / (R0 * 2.0 ** -20)) * (R0 * 2.0 ** -20)
    return p + R0 * np.array([2.0 ** m_, -(2.0 ** (m_ - 1)), 2.0 ** (m_ - 2)]), m


CLOUDS = {"gauss_%d" % n: (lambda n=n: _gauss(n, 100 + n)) for n in (2, 65, 257, 1000, 5003)}
CLOUDS.update({"heavy_tail": _heavy_tail, "zero_mass_30pc": _zero_scattered, "gauss_5003_shift_20": lambda: _shifted(20)})
_cloud_cache = {}


def _cloud(name):
    """(points, mass, eps, reference rows, row scales), computed once and left unchanged"""
    if name not in _cloud_cache:
        p, m = CLOUDS[name]()
        p, m = np.ascontiguousarray(p), np.ascontiguousarray(m)
        D = np.linalg.norm(p.max(axis=0) - p.min(axis=0))
        eps = EPS_OVER_D * D
        ref, scale = _direct(p, m, eps)
        for a in (p, m, ref, scale):
            a.setflags(write=False)
        _cloud_cache[name] = (p, m, eps, ref, scale)
    return _cloud_cache[name]


def _splits(p):
    """name -> labels: halves by the x median, 8 parts by bisection, random labels 0..3 (coinciding boxes), one part of a
    single particle, a label nobody carries"""
    import sph_code_amd.multigpu as mg
    n = len(p)
    rs = np.random.RandomState(n)
    lone = np.zeros(n, np.int32)
    lone[n // 2] = 1
    gap = (p[:, 1] > np.median(p[:, 1])).astype(np.int32) * 2              # labels 0 and 2: part 1 is empty
    return {"halves": (p[:, 0] > np.median(p[:, 0])).astype(np.int32),
            "rcb8": mg.rcb_regions(p, 8)[0].astype(np.int32),
            "random4": rs.randint(0, 4, n).astype(np.int32),
            "lone": lone,
            "empty_label": gap}


def _parts(m, p, eps, lab, ws, order, counts=False):
    import sph_code_amd.compat as nsc
    return nsc.grav_force_tree_parts(m, p, np.full(len(m), float(eps)), lab, G=G, ws=ws, order=order, return_counts=counts)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_gpu_parts_count_every_source_once(name):
    """Every split of every cloud, order 1 and 2, ws 1 and 2: each row within (4 (D/eps)^2 + 1e-12) of its scale of the
    oracle's direct sum at eps = 1e6 D - no source dropped, none doubled, across the export and the remote sum; two calls
    give the same bits.  For N = 5003 at ws = 1 (the default): the halves send cells and fewer particles than they hold;
    random labels (the parts' boxes coincide, so no cell is clear of them) send at least 90 % of each part as particles.
    (A regime check, not a measurement.  At ws = 2 a half of 2500 particles is about three and a half level-1 cells wide,
    and a cell must stand two of its edges clear of the other half: measured here, the half x > median still sends cells
    to the other, the half x < median sends [0 cells, 2502 particles] - the rule as it is defined, so ws = 2 is held to
    the row bound and to reproducibility, not to a count.)"""
    p, m, eps, ref, scale = _cloud(name)
    bad = []
    for sname, lab in _splits(p).items():
        for order in (1, 2):
            for ws in (1, 2):
                got, cnt = _parts(m, p, eps, lab, ws, order, counts=True)
                miss = ~(np.abs(got - ref) <= TOL_LIMIT * scale)              # (a NaN misses)
                if miss.any():
                    with np.errstate(all="ignore"):
                        worst = np.nanmax(np.where(scale > 0, np.abs(got - ref) / scale, 0.0))
                    bad.append((sname, order, ws, "%d rows" % miss.any(axis=1).sum(), "worst %.3g" % worst))
                again = _parts(m, p, eps, lab, ws, order)
                if again.tobytes() != got.tobytes():
                    bad.append((sname, order, ws, "two calls differ"))
                if name == "gauss_5003" and ws == 1:
                    size = np.bincount(lab, minlength=cnt.shape[0])
                    for a in range(cnt.shape[0]):
                        for b in range(cnt.shape[0]):
                            if a == b or size[a] == 0 or size[b] == 0:
                                continue
                            if sname == "halves" and not (cnt[a, b, 0] > 0 and cnt[a, b, 1] < size[a]):
                                bad.append((sname, order, ws, "counts", a, b, cnt[a, b].tolist()))
                            if sname == "random4" and not cnt[a, b, 1] >= 0.9 * size[a]:
                                bad.append((sname, order, ws, "counts", a, b, cnt[a, b].tolist(), int(size[a])))
    assert not bad, "\n".join(map(str, bad))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["gauss_257", "gauss_5003", "heavy_tail"])
def test_gpu_one_part_is_the_single_domain_tree(name):
    import sph_code_amd.compat as nsc
    p, m, eps, _, _ = _cloud(name)
    h = np.full(len(m), eps)
    for order in (1, 2):
        for ws in (1, 2):
            one = _parts(m, p, eps, np.zeros(len(m), np.int32), ws, order)
            assert one.tobytes() == nsc.grav_force_tree(m, p, h, G=G, ws=ws, order=order).tobytes(), (order, ws)


@pytest.mark.gpu
@pytest.mark.parametrize("e_over_d", [0.0, 0.5])
def test_gpu_remote_multipole_term(e_over_d):
    """The bar cluster B (part 0) reaches the 600 targets of part 1 as exactly ONE cell record and no particle, at
    ws 1 and 2: order 1 within the C_1 bound and order 2 within the C_2 bound on every target row, order 1 beyond the
    order-2 bound on at least half of them."""
    p, m, b, dist, lab = _bar_and_balls()
    eps = e_over_d * b / 0.03
    ref, scale = _direct(p, m, eps)
    ref, slack = ref[NB:], 1e-12 * np.linalg.norm(scale[NB:], axis=1)
    bound1, bound2 = _bar_bounds(m, b, dist, eps)
    bad = []
    for ws in (1, 2):
        err = {}
        for order in (1, 2):
            got, cnt = _parts(m, p, eps, lab, ws, order, counts=True)
            assert cnt[0, 1].tolist() == [1, 0], (ws, order, cnt.tolist())
            assert cnt[1, 0].tolist() == [0, 0], (ws, order, cnt.tolist())
            assert np.isfinite(got).all()
            err[order] = np.linalg.norm(got[NB:] - ref, axis=1)
        print("eps/d %.1f ws %d: order 1 up to %.3f of its bound, order 2 up to %.4f; order 1 beyond the order-2 bound on "
              "%.2f of the rows" % (e_over_d, ws, (err[1] / bound1).max(), (err[2] / bound2).max(),
                                    (err[1] > bound2 + slack).mean()))
        if not (err[1] <= bound1 + slack).all():
            bad.append((ws, "order 1", (err[1] / bound1).max()))
        if not (err[2] <= bound2 + slack).all():
            bad.append((ws, "order 2", (err[2] / bound2).max()))
        if not (err[1] > bound2 + slack).mean() >= 0.5:
            bad.append((ws, "order 1 within the order-2 bound", (err[1] > bound2 + slack).mean()))
    assert not bad, "\n".join(map(str, bad))


def _oracle_direct_rows(p, m, eps, chunk=16):
    """orc.gravity_direct(p, m, eps, return_abs=True) at G = 6.67430e-11, term by term the oracle's own expression, axis by
    axis in cache-sized pieces on the tensor library's CPU threads (the oracle's (512, n, 3) NumPy temporaries take 40 s
    at n = 30000, this a few)."""
    import torch
    P, M = torch.from_numpy(np.ascontiguousarray(p.T)), torch.from_numpy(m)
    n = len(m)
    out, out_abs = torch.zeros((3, n), dtype=torch.float64), torch.zeros((3, n), dtype=torch.float64)
    e2 = float(eps) ** 2
    for a in range(0, n, chunk):
        d = [P[c][None, :] - P[c][a:a + chunk, None] for c in range(3)]
        r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + e2
        w = torch.where(r2 > 0, M[None, :] / (r2 * torch.sqrt(r2)), torch.zeros_like(r2))
        for c in range(3):
            t = w * d[c]
            out[c, a:a + chunk] = G * t.sum(dim=1)
            out_abs[c, a:a + chunk] = G * t.abs().sum(dim=1)
    return np.ascontiguousarray(out.T.numpy()), np.ascontiguousarray(out_abs.T.numpy())


def test_cpu_oracle_restatement_is_the_oracle():
    from oracle import sph_oracle as orc
    p, m = _gauss(700, 3)
    p[5] = p[9]                                                      # (a coincident pair)
    for eps in (0.0, 3e4 * AU):
        ref, scale = orc.gravity_direct(p, m, eps, G=G, return_abs=True)
        got, got_scale = _oracle_direct_rows(p, m, eps)
        assert (np.abs(got - ref) <= 1e-14 * scale).all() and np.allclose(got_scale, scale, rtol=1e-13, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("workload", ["polytrope", "uniform_cube"])
def test_gpu_parts_accuracy_on_real_clouds(workload):
    """2 and 8 bisection parts of 30000 particles against the exact sum: the rms gates the single-domain tree is held to
    (order 2: 4e-3 at ws 1, 6e-4 at ws 2; order 1: 3e-2, 6e-3), the error falling as ws grows; ws = 0 (everything travels
    as particles) is the exact sum, row by row within 1e-12 of the row's scale of the oracle."""
    import sph_code_amd.compat as nsc
    import sph_code_amd.ics as ics
    import sph_code_amd.multigpu as mg
    from scipy.spatial import cKDTree
    s = ics.WORKLOADS[workload](30000)
    p = np.ascontiguousarray(s["points"])
    m = np.ascontiguousarray(s["mass"] * np.random.RandomState(1).uniform(0.5, 1.5, 30000))
    h = cKDTree(p).query(p, k=40)[0][:, -1]
    ref = nsc.grav_force_direct(m, p, h)
    scale = np.sqrt(np.mean(np.sum(ref ** 2, axis=1)))
    exact, exact_scale = _oracle_direct_rows(p, m, np.median(h))
    for world in (2, 8):
        lab = mg.rcb_regions(p, world)[0].astype(np.int32)
        for order, bounds in ((1, ((1, 3e-2), (2, 6e-3))), (2, ((1, 4e-3), (2, 6e-4)))):
            last = None
            for ws, bound in bounds:
                a = nsc.grav_force_tree_parts(m, p, h, lab, ws=ws, order=order)
                err = np.sqrt(np.mean(np.sum((a - ref) ** 2, axis=1))) / scale
                print("%s, %d parts, order %d, ws %d: rms error %.3g (gate %.3g)" % (workload, world, order, ws, err, bound))
                assert err < bound, (world, order, ws, err)
                assert last is None or err < last
                last = err
        a0 = nsc.grav_force_tree_parts(m, p, h, lab, ws=0)
        worst = np.max(np.abs(a0 - exact) / exact_scale)
        assert worst <= 1e-12, (world, worst)


@pytest.mark.gpu
def test_gpu_remote_kernel_tile_and_target_edges():
    """ws = 0 with two parts: source part sizes around the record tile (256) and target part sizes around a wave and a
    workgroup - every row within 1e-12 of its scale of the oracle, unsoftened, with one particle of the source part
    sitting exactly on one of the target part (finite; the pair contributes nothing, as in the direct kernel)."""
    rs = np.random.RandomState(77)
    bad = []
    for ns in (1, 255, 256, 257, 513):
        for nt in (1, 63, 64, 65, 257):
            p = rs.normal(size=(ns + nt, 3)) * 1e5 * AU
            p[:ns, 0] -= 1e5 * AU
            p[ns + nt - 1] = p[ns - 1]                                         # a coincident pair across the parts
            m = rs.uniform(0.5, 2.0, ns + nt) * 1e-3 * SOLAR
            lab = np.append(np.zeros(ns, np.int32), np.ones(nt, np.int32))
            p = np.ascontiguousarray(p)
            ref, scale = _direct(p, m, 0.0)
            got, cnt = _parts(m, p, 0.0, lab, 0, 2, counts=True)
            if cnt[0, 1].tolist() != [0, ns] or cnt[1, 0].tolist() != [0, nt]:
                bad.append((ns, nt, "counts", cnt.tolist()))
            if not (np.isfinite(got).all() and (np.abs(got - ref) <= 1e-12 * scale).all()):
                with np.errstate(all="ignore"):
                    bad.append((ns, nt, float(np.nanmax(np.abs(got - ref) / scale))))
    assert not bad, "\n".join(map(str, bad))


@pytest.mark.gpu
def test_gpu_parts_and_device_entries_check_their_arguments():
    """SPHX_E_ARG / SPHX_E_STATE with a message, as the neighbouring entry points give them."""
    import torch
    import sph_code_amd.compat as nsc
    import sph_code_amd.multigpu as mg
    p, m = _gauss(100, 1)
    h = np.full(100, 1e15)
    lab = np.zeros(100, np.int32)
    with pytest.raises(ValueError, match="ws="):
        nsc.grav_force_tree_parts(m, p, h, lab, ws=5)
    with pytest.raises(ValueError, match="one label per particle"):
        nsc.grav_force_tree_parts(m, p, h, lab[:50])
    bad = lab.copy()
    bad[7] = -1
    with pytest.raises(ValueError, match="part_of"):
        nsc.grav_force_tree_parts(m, p, h, bad)
    be = mg.LibBackend(0, k=16)
    pos = torch.as_tensor(p, device="cuda:0")
    mass = torch.as_tensor(m, device="cuda:0")
    with pytest.raises(RuntimeError, match="sphx_dev_search"):
        be.gravity_build(pos, mass, 100, [0.0, 0.0, 0.0])
    be.search(pos, 100, None, 0.0)
    be._grav_no = 100
    with pytest.raises(RuntimeError, match="sphx_dev_gravity_build"):
        be.gravity_local(1, G, 1e15)
    with pytest.raises(ValueError, match="not finite"):
        be.gravity_build(pos, mass, 100, [float("nan"), 0.0, 0.0])
    be.gravity_build(pos, mass, 100, [0.0, 0.0, 0.0])
    with pytest.raises(ValueError, match="ws="):
        be.gravity_local(7, G, 1e15)
    boxes = torch.zeros((2, 6), dtype=torch.float64, device="cuda:0")
    with pytest.raises(ValueError, match="rank"):
        be.gravity_export(boxes, 2, 1, 0, 0)
    be.search(pos, 100, None, 0.0)                        # a new search: the pyramid of the old one is gone
    with pytest.raises(RuntimeError, match="sphx_dev_gravity_build"):
        be.gravity_export(boxes, 0, 1, 0, 0)
    torch.cuda.synchronize()
