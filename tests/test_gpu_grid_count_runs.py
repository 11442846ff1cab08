"""The fused step's cell count with one histogram atomic per run of same-cell particles (grid_count_fused, sphx_grid.hip;
sphx_runs.h).  Whole steps on clouds built around the run rule's edges, compared bit for bit with
the same cloud stepped with SPHX_BLOB=0 (the per-cell sort kernel, no blob order) and with SPHX_KNN_GROUP=0 (the general
search) - three steps at the fixed dt of 1e-30 of tests/test_gpu_grid_order.py, so that one differing bit is not amplified:
the positions stay put and the second and third step's count sees the state in the first one's cell order, a cell's
members in consecutive threads.  (The first step after an upload sizes its grid by a reduction of its own and counts
with cell_count, so the A B A B upload order of case c is sorted before the step's fused count sees it; orders that are
not cell-contiguous reach the rule in the host replay, tests/test_grid_runs_cpu.py, and reach the kernel where a caller's
own order goes through a lagged build - the second sphx_dev_search of a context: the last test here.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ("points", "velocities", "sizes")
DT = 1e-30


def _state(pts, vel=None):
    import sph_code_amd.ics as ics
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    s0 = ics.WORKLOADS["uniform_cube"](len(pts))
    s0["points"] = pts
    s0["velocities"] = np.zeros_like(pts) if vel is None else np.ascontiguousarray(vel, dtype=np.float64)
    return s0


def _run(s0, K, dts):
    """One download per entry of dts; a fresh context reads the switches."""
    from sph_code_amd.sim import Simulation
    sim = Simulation(s0, n_neigh=K)
    out = []
    for dt in dts:
        sim.step(1, fixed_dt=dt)
        out.append(sim.download())
    return out, sim


def _one_cell(n):
    """n - 40 particles within 1e7 m of one point, and two far corner groups of 20 that size the box (mean +- 3 sigma: some
    1e16 m a side, whose cells - at least 1e-4 of it, and no more than 32 n + 1024 of them - are 1e14 m and up).  Groups,
    not single particles: a lone corner particle sees the whole cluster at one distance to nine digits, its K = 16
    nearest are a matter of the search's near-tie rule, and its acceleration then differs between the search's forms by
    per cent - before this kernel changed as after (measured on both libraries); with 19 mates a few 1e6 m away its
    neighbours are its own group."""
    rs = np.random.RandomState(n)
    pts = np.array([1.37e14, -0.71e14, 2.23e14]) + (rs.rand(n, 3) - 0.5) * 1e7
    lo, hi = np.arange(n // 3, n // 3 + 20), np.arange(2 * n // 3, 2 * n // 3 + 20)
    pts[lo] += np.array([-1.0e16, -1.1e16, -0.9e16]) - pts[0]
    pts[hi] += np.array([1.1e16, 0.9e16, 1.0e16]) - pts[0]
    return pts


def _lattice(twins):
    m = 16
    ax = (np.arange(m) - (m - 1) / 2.0) * 1e16
    pts = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3)
    return np.concatenate([pts, pts[::8]]) if twins else pts


def _two_cells_alternating(n):
    rs = np.random.RandomState(7)
    pts = (rs.rand(n, 3) - 0.5) * 1e7
    pts[0::2] += [-1.0e16, -0.9e16, -1.1e16]           # A B A B ... in storage order
    pts[1::2] += [1.1e16, 1.0e16, 0.9e16]
    return pts


CLOUDS = {
    "a_one_cell_300": lambda: _one_cell(300),                    # runs fill whole waves, cut at the waves' ends; below CELL_SORT_WAVE
    "a_one_cell_700": lambda: _one_cell(700),                    # ... and above it: the cell keeps its arrival order
    "b_lattice": lambda: _lattice(False),                        # every run of length 1
    "b_lattice_twins": lambda: _lattice(True),                   # every 8th particle twice: coincident points, runs of 2
    "c_alternating_1000": lambda: _two_cells_alternating(1000),  # not a multiple of 64 or 256; equal cells never adjacent at upload
    "d_last_wave_of_one": lambda: np.random.RandomState(193).rand(64 * 3 + 1, 3) * 1e17,
}


@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_step_equals_storage_order_and_general_search(name, monkeypatch):
    pts = CLOUDS[name]()
    K = 16
    got, _ = _run(_state(pts), K, [DT] * 3)
    for var in ("SPHX_BLOB", "SPHX_KNN_GROUP"):
        monkeypatch.setenv(var, "0")
        ref, _ = _run(_state(pts), K, [DT] * 3)
        monkeypatch.delenv(var)
        for it in range(3):
            for key in KEYS:
                assert np.array_equal(got[it][key], ref[it][key], equal_nan=True), (name, var, it, key)
    assert np.array_equal(got[2]["points"], pts)                 # (nothing moved: the cells are those of the upload)


@pytest.mark.parametrize("n", [1000, 64 * 3 + 1])
def test_fused_count_on_the_callers_alternating_order(n):
    """Case c on the kernel itself.  sphx_dev_search builds its grid on the caller's order; the second search of a context
    sizes the grid from the first one's statistics and counts with grid_count_fused - on two cells whose members alternate
    in storage, A B A B ...: equal cells that are never adjacent, every run of length 1, at n = 1000 and with a last wave
    of one lane.  The radii must be the first search's bit for bit (that one counts with cell_count) and the exact K-th
    neighbour distances to the 2e-15 tests/test_gpu_parity.py holds kNN distances to."""
    import torch
    from oracle import sph_oracle as orc
    from sph_code_amd import multigpu as mg
    K = 16
    pts = np.ascontiguousarray(_two_cells_alternating(n))
    _, _, _, _, h_ref = orc.neighbors(pts, np.inf, K, eps=0.0)
    be = mg.LibBackend(0, k=K)
    pos = torch.as_tensor(pts, device="cuda:0")
    h0 = be.search(pos, n, None, 0.0).cpu().numpy().copy()
    np.testing.assert_allclose(h0, h_ref, rtol=2e-15, atol=0)
    for _ in range(2):
        h1 = be.search(pos, n, None, 0.0).cpu().numpy()
        assert np.array_equal(h1, h0)
    torch.cuda.synchronize()
