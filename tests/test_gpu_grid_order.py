"""The fused step's grid build without its pass over the cells (sphx_grid.hip, sphx_integrate.hip): the scatter writes
the blob order's curve counts, the gather that permutes the state puts every cell's members in order by counting, and
the host's two cues are counted beside the search.  The finished orders must be those of the per-cell pass, element for
element - compared on the device by sphx_selftest_grid_order - and a run of the step must not notice."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CELL_SORT_SERIAL, CELL_SORT_WAVE = 16, 512      # sphx_internal.h


def _cell_counts(pts, cell):
    """Members per non-empty cell of the grid the library builds on pts: origin at the cloud's minimum, cells of `cell`
    (valid where the cloud lies within mean +- 3 sigma and the cell count stays below the cap: the callers' clouds)."""
    idx = np.floor((pts - pts.min(axis=0)) / cell).astype(np.int64)
    _, cnt = np.unique(idx, axis=0, return_counts=True)
    return cnt


def _selftest(pts, cell):
    from sph_code_amd import _lib
    ctx = _lib.Context()
    x, y, z = (np.ascontiguousarray(pts[:, c], dtype=np.float64) for c in range(3))
    dp = C.POINTER(C.c_double)
    bad, taken = C.c_longlong(-1), C.c_int(-1)
    for _ in range(2):                 # (twice on one context: the second build finds the first one's buffers and state)
        rc = ctx.lib.sphx_selftest_grid_order(ctx.h, len(pts), x.ctypes.data_as(dp), y.ctypes.data_as(dp), z.ctypes.data_as(dp),
                                              float(cell), C.byref(bad), C.byref(taken))
        assert rc == 0, ctx.lib.sphx_last_error(ctx.h)
        assert bad.value == 0, bad.value
        assert taken.value == 1
    ctx.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 5000])
def test_order_by_counting_on_a_uniform_cube(n):
    """About 1.6 particles per cell: empty cells everywhere, the others hold a handful.  n = 1: one cell; 63 / 64 / 65: around a
    wave; 5000: twenty blocks of the scatter and the gather."""
    pts = np.random.RandomState(n).rand(n, 3)
    cell = (1.6 / n) ** (1.0 / 3.0)
    if n == 5000:
        cnt = _cell_counts(pts, cell)
        assert cnt.max() > 1 and len(cnt) < (1.0 / cell) ** 3                 # (members to order; empty cells among them)
    _selftest(pts, cell)


def test_order_by_counting_on_a_gaussian_cloud():
    """Cells of 2 .. 16 members (one lane's insertion sort in the per-cell pass) and a few of 17 .. 512 (the wave's rank sort)."""
    pts = np.random.RandomState(11).normal(size=(5000, 3))
    cell = 0.45
    cnt = _cell_counts(pts, cell)
    assert ((cnt >= 2) & (cnt <= CELL_SORT_SERIAL)).sum() > 100
    assert ((cnt > CELL_SORT_SERIAL) & (cnt <= CELL_SORT_WAVE)).sum() >= 3
    _selftest(pts, cell)


@pytest.mark.parametrize("m", [16, 17, 512, 513])
def test_order_by_counting_at_the_size_class_boundaries(m):
    """One cell of exactly m members, jittered inside it, in a cloud of 300: the last size the serial sort takes, the first
    and the last the wave takes, and the first that keeps its arrival order."""
    rs = np.random.RandomState(100 + m)
    cell, centre = 0.1, 0.45
    spread = rs.rand(2000, 3)
    spread = spread[np.max(np.abs(spread - centre), axis=1) > 0.1][:300]      # (none of them in or beside the forced cell)
    assert len(spread) == 300
    members = centre + (rs.rand(m, 3) - 0.5) * 2e-3
    pts = np.concatenate([spread, members])
    pts = np.ascontiguousarray(pts[rs.permutation(len(pts))])                 # (members' indices interleaved with the others')
    cnt = _cell_counts(pts, cell)
    assert cnt.max() == m and (cnt == m).sum() == 1
    _selftest(pts, cell)


def test_arrival_order_stays_above_the_cap():
    """700 coincident particles: one cell over CELL_SORT_WAVE, whose members keep the order of the scatter in both forms."""
    pts = np.full((700, 3), 0.25)
    _selftest(pts, 0.1)


def test_order_by_counting_with_particles_clamped_into_boundary_cells():
    """100 of 2000 particles far outside the box of mean +- 3 sigma: they land in the grid's boundary cells."""
    rs = np.random.RandomState(5)
    core = rs.rand(1900, 3)
    u = rs.normal(size=(100, 3))
    far = 0.5 + u / np.linalg.norm(u, axis=1)[:, None] * rs.uniform(3.0, 6.0, 100)[:, None]
    pts = np.concatenate([core, far])
    sig = pts.std(axis=0)
    assert (np.abs(far - pts.mean(axis=0)) > 3.0 * sig).any(axis=1).sum() >= 50     # (outside the robust box)
    pts = np.ascontiguousarray(pts[rs.permutation(len(pts))])
    _selftest(pts, (1.6 / 1900) ** (1.0 / 3.0))


def _lattice_state():
    import sph_code_amd.ics as ics
    m = 16
    ax = (np.arange(m) - (m - 1) / 2.0) * 1e16
    pts = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3)
    pts = np.ascontiguousarray(np.concatenate([pts, pts[::8]]))              # every 8th particle twice: coincident pairs
    s0 = ics.WORKLOADS["uniform_cube"](len(pts))
    s0["points"] = pts
    s0["velocities"] = np.zeros_like(pts)
    return s0


def _run_lattice(steps=3, K=16):
    """Three steps at a fixed dt of 1e-30, as in test_hinted_search_on_a_lattice_with_exact_ties_and_coincident_particles:
    the positions stay put, the velocities are the accelerations x dt - with K = 16 cutting through a shell of exact
    ties, and pairs at distance 0, they depend on which of the tied neighbours the search keeps, that is on the order of a
    cell's members.  (Under the reference's dt rule the coincident pairs throw each other out - the oracle's cloud is nine
    times its size after the third step - and one run of the whole suite saw two such runs differ, which no run since
    has shown again, on this build or the one before it)"""
    from sph_code_amd.sim import Simulation
    sim = Simulation(_lattice_state(), n_neigh=K)       # a fresh context reads the switches
    for _ in range(steps):
        sim.step(1, fixed_dt=1e-30)
    return sim.download()


@pytest.fixture(scope="module")
def lattice_default():
    return _run_lattice()


def test_step_on_a_lattice_with_coincident_pairs_repeats(lattice_default):
    """Exact ties everywhere and cells of several members: the second and third step order the members in the gather."""
    again = _run_lattice()
    for key in ("points", "velocities", "sizes"):
        assert np.array_equal(lattice_default[key], again[key]), key


def test_step_on_a_lattice_equals_storage_order(lattice_default, monkeypatch):
    """SPHX_BLOB=0 keeps the per-cell sort kernel and builds no blob order: the same trajectory, bit for bit."""
    monkeypatch.setenv("SPHX_BLOB", "0")
    ref = _run_lattice()
    monkeypatch.delenv("SPHX_BLOB")
    for key in ("points", "velocities", "sizes"):
        assert np.array_equal(lattice_default[key], ref[key]), key
