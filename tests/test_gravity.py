"""Self-gravity: softened direct summation.

The reference's tree gravity (nsc:252-415) cannot be run here and has no golden vectors: parity with it is
UNPINNED.  What is tested is the sum it approximates (softening as nsc:358,385): the oracle against closed
forms, the HIP kernel against the oracle, and the step loop with gravity against the oracle's step."""
import numpy as np
import pytest

AU = 149597870700.0
SOLAR = 1.989e30


def _cloud(n, seed=3):
    rs = np.random.RandomState(seed)
    p = rs.normal(size=(n, 3)) * 1e5 * AU
    m = rs.uniform(0.5, 2.0, n) * 1e-3 * SOLAR
    h = rs.uniform(0.5, 1.5, n) * 2e4 * AU
    return p, m, h


def test_oracle_two_bodies_closed_form():
    from oracle import sph_oracle as orc
    d, eps = 3.0e12, 1.0e12
    p = np.array([[0., 0., 0.], [d, 0., 0.]])
    m = np.array([2.0e30, 5.0e29])
    a = orc.gravity_direct(p, m, eps)
    f = orc.G_NEWTON / (d * d + eps * eps) ** 1.5 * d
    np.testing.assert_allclose(a[0], [f * m[1], 0, 0], rtol=1e-14, atol=0)
    np.testing.assert_allclose(a[1], [-f * m[0], 0, 0], rtol=1e-14, atol=0)
    # unsoftened, coincident points contribute nothing
    a0 = orc.gravity_direct(np.vstack([p, p[:1]]), np.append(m, 1e30), 0.0)
    assert np.isfinite(a0).all()


def test_oracle_momentum_and_shell_theorem():
    from oracle import sph_oracle as orc
    p, m, h = _cloud(1500)
    a = orc.gravity_direct(p, m, np.median(h))
    net = np.abs((a * m[:, None]).sum(axis=0)).max()
    assert net <= 1e-12 * np.abs(a * m[:, None]).sum()          # pairwise forces cancel
    # far field of the whole cloud = a point mass at its centre of mass
    far = np.array([[5e9 * AU, 0., 0.]])
    com = (p * m[:, None]).sum(axis=0) / m.sum()
    aa = orc.gravity_direct(np.vstack([p, far]), np.append(m, 0.0), np.median(h))[-1]
    d = com - far[0]
    point = orc.G_NEWTON * m.sum() * d / np.linalg.norm(d) ** 3
    assert np.linalg.norm(aa - point) <= 1e-6 * np.linalg.norm(point)


@pytest.mark.gpu
def test_gpu_direct_sum_vs_oracle():
    from oracle import sph_oracle as orc
    import sph_code_amd.compat as nsc
    for n in (1, 2, 255, 257, 3000):
        p, m, h = _cloud(n, seed=n)
        got = nsc.grav_force_direct(m, p, h)
        ref = orc.gravity_direct(p, m, np.median(h))
        scale = np.max(np.abs(ref)) if n > 1 else 1.0
        assert np.max(np.abs(got - ref)) <= 1e-12 * scale, n
    net = np.abs((got * m[:, None]).sum(axis=0)).max()
    assert net <= 1e-11 * np.abs(got * m[:, None]).sum()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [255, 256, 257, 511, 512, 513, 3000])
def test_gpu_direct_sum_rows_vs_oracle(n):
    """Row by row around the source tile (256): every component within 1e-12 of the sum of its terms'
    magnitudes - a global max|ref| hides a row whose terms cancel."""
    from oracle import sph_oracle as orc
    import sph_code_amd.compat as nsc
    p, m, h = _cloud(n, seed=n)
    got = nsc.grav_force_direct(m, p, h)
    ref, scale = orc.gravity_direct(p, m, np.median(h), return_abs=True)
    assert (np.abs(got - ref) <= 1e-12 * scale).all(), np.max(np.abs(got - ref) / scale)


def _direct_c_abi(m, p, sizes, eps):
    from sph_code_amd import _lib
    dp = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data_as(_lib.c_double_p)
    m, p = np.ascontiguousarray(m), np.ascontiguousarray(p)
    sizes = None if sizes is None else np.ascontiguousarray(sizes)
    c = _lib.Context()
    out = np.full((len(m), 3), np.nan)
    c.check(c.lib.sphx_gravity_direct(c.h, len(m), dp(m), dp(p), dp(sizes), float(eps), 6.67430e-11, dp(out)))
    c.close()
    return out


@pytest.mark.gpu
def test_gpu_direct_sum_unsoftened_coincident_pairs():
    """eps = 0 by value (sizes = NULL) with 40 coincident pairs: a pair at zero distance contributes
    nothing, and every row stays within 1e-12 of its scale."""
    from oracle import sph_oracle as orc
    p, m, _ = _cloud(600, seed=77)
    p[40:80] = p[:40]
    got = _direct_c_abi(m, p, None, 0.0)
    ref, scale = orc.gravity_direct(p, m, 0.0, return_abs=True)
    assert np.isfinite(got).all()
    assert (np.abs(got - ref) <= 1e-12 * scale).all(), np.max(np.abs(got - ref) / scale)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [512, 513])
def test_gpu_direct_sum_softening_is_the_median_of_sizes(n):
    """sizes given: eps is their median as NumPy defines it (even n: the mean of the two middle values),
    taken on the device - h spread over a factor 10^6, with ties, some of them at the middle."""
    from oracle import sph_oracle as orc
    p, m, _ = _cloud(n, seed=n)
    rs = np.random.RandomState(n + 1)
    h = 2e4 * AU * 10.0 ** rs.uniform(-3.0, 3.0, n)
    h[::7] = h[3]
    h[1], h[2] = 2e1 * AU, 2e7 * AU
    order = np.argsort(h)
    if n % 2:
        h[order[[n // 2 - 1, n // 2 + 1]]] = h[order[n // 2]]               # ties at the middle value
    else:
        h[order[[n // 2 - 3, n // 2 - 2]]] = h[order[n // 2 - 1]]           # ties up to the lower middle value
    srt = np.sort(h)
    assert h.max() / h.min() == 1e6 and len(np.unique(h)) < n - 50
    if n % 2:
        assert srt[n // 2 - 1] == srt[n // 2] == srt[n // 2 + 1]
    else:
        assert srt[n // 2 - 3] == srt[n // 2 - 1] != srt[n // 2]
    got = _direct_c_abi(m, p, h, 0.0)
    ref, scale = orc.gravity_direct(p, m, np.median(h), return_abs=True)
    assert (np.abs(got - ref) <= 1e-12 * scale).all(), np.max(np.abs(got - ref) / scale)


@pytest.mark.gpu
def test_gpu_step_with_gravity_vs_oracle():
    """6 leapfrog steps of a small polytrope with self-gravity on: rtol 1e-9 on x, v, a vs the oracle's step
    (gravity = direct sum, eps = median(h) of each step)."""
    from oracle import sph_oracle as orc
    import sph_code_amd.ics as ics
    from sph_code_amd.sim import Simulation
    n, K, nsteps = 3000, 40, 6
    s0 = ics.polytrope_sphere(n)
    Gbig = 3e7 * orc.G_NEWTON          # this light test cloud would hardly feel its own gravity otherwise
    sim = Simulation(s0, n_neigh=K, gravity="direct", G=Gbig)
    plain = Simulation(s0, n_neigh=K)
    sim.ctx.set_timing_detail(True)          # (per-pass timing events: ms_gravity below)
    plain.ctx.set_timing_detail(True)
    ref = dict(s0)
    for it in range(nsteps):
        sim.step(1)
        plain.step(1)
        ref = orc.step(ref, n_neigh=K, eps=0.0, first=(it == 0), with_gravity=True, grav_G=Gbig)
    got = sim.download()
    L = np.max(np.abs(ref["points"])); V = np.max(np.abs(ref["velocities"])); A = np.max(np.abs(ref["total_accel"]))
    assert np.max(np.abs(got["points"] - ref["points"])) <= 1e-9 * L
    assert np.max(np.abs(got["velocities"] - ref["velocities"])) <= 1e-9 * V
    assert np.max(np.abs(got["total_accel"] - ref["total_accel"])) <= 1e-9 * A
    # gravity really is in the acceleration
    assert np.max(np.abs(got["total_accel"] - plain.download()["total_accel"])) > 1e-3 * A
    assert sim.stats()["ms_gravity"] > 5.0 * plain.stats()["ms_gravity"]       # the latter: an empty event gap


@pytest.mark.gpu
@pytest.mark.parametrize("workload", ["polytrope", "uniform_cube"])
def test_gpu_tree_vs_direct_sum(workload):
    """Cell-pyramid multipoles (sphx_gravity_tree) against the exact sum: the force error is set by the
    separation parameter ws and the order - monopoles: rms 0.4-1.3 % at ws = 1, 0.06-0.3 % at ws = 2, < 0.1 %
    at ws = 3; with the second moments (order 2, the softened kernel's own expansion) ws = 1 already gives
    0.07-0.13 %, ws = 2 0.01 %."""
    import sph_code_amd.compat as nsc
    import sph_code_amd.ics as ics
    from scipy.spatial import cKDTree
    s = ics.WORKLOADS[workload](30000)
    p, m = s["points"], s["mass"] * np.random.RandomState(1).uniform(0.5, 1.5, 30000)
    h = cKDTree(p).query(p, k=40)[0][:, -1]
    ref = nsc.grav_force_direct(m, p, h)
    scale = np.sqrt(np.mean(np.sum(ref ** 2, axis=1)))
    for order, bounds in ((1, ((1, 3e-2), (2, 6e-3), (3, 3e-3))), (2, ((1, 4e-3), (2, 6e-4), (3, 3e-4)))):
        last = None
        for ws, bound in bounds:
            a = nsc.grav_force_tree(m, p, h, ws=ws, order=order)
            err = np.sqrt(np.mean(np.sum((a - ref) ** 2, axis=1))) / scale
            assert err < bound, (order, ws, err)
            assert last is None or err < last          # wider separation, smaller error
            last = err
    # the default (order 2, ws 1) is at least as good as monopoles at ws 2
    e_def = np.sqrt(np.mean(np.sum((nsc.grav_force_tree(m, p, h) - ref) ** 2, axis=1))) / scale
    e_m2 = np.sqrt(np.mean(np.sum((nsc.grav_force_tree(m, p, h, ws=2, order=1) - ref) ** 2, axis=1))) / scale
    assert e_def < 1.5 * e_m2, (e_def, e_m2)
    # degenerate grids: a handful of particles, all in one place
    for n in (1, 2, 9):
        q = p[:n]
        np.testing.assert_allclose(nsc.grav_force_tree(m[:n], q, h[:n]), nsc.grav_force_direct(m[:n], q, h[:n]),
                                   rtol=1e-12, atol=0)


@pytest.mark.gpu
def test_gpu_step_tree_gravity_tracks_direct():
    import sph_code_amd.ics as ics
    from sph_code_amd.sim import Simulation
    from oracle import sph_oracle as orc
    s0 = ics.polytrope_sphere(20000)
    Gbig = 3e7 * orc.G_NEWTON
    a = Simulation(s0, n_neigh=40, gravity="direct", G=Gbig)
    b = Simulation(s0, n_neigh=40, gravity="tree", G=Gbig)
    c = Simulation(s0, n_neigh=40)
    b.ctx.set_timing_detail(True)
    for sim in (a, b, c):
        sim.step(3)
    ra, rb, rc = a.download(), b.download(), c.download()
    grav = ra["total_accel"] - rc["total_accel"]                 # what gravity adds
    gs = np.sqrt(np.mean(np.sum(grav ** 2, axis=1)))
    assert gs > 0.1 * np.sqrt(np.mean(np.sum(rc["total_accel"] ** 2, axis=1)))
    diff = np.sqrt(np.mean(np.sum((rb["total_accel"] - ra["total_accel"]) ** 2, axis=1)))
    assert diff < 1e-2 * gs
    assert b.stats()["ms_gravity"] > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("workload,n", [("polytrope", 30000), ("uniform_cube", 9000), ("polytrope", 70)])
def test_gpu_tree_wave_kernel_is_the_per_thread_walk(workload, n, monkeypatch):
    """The wave-cooperative LDS form of the tree walk adds every lane's terms in the order of the
    per-thread walk (SPHX_GRAV_KERNEL=0) - the same sum up to how the compiler contracts the two loops'
    multiply-adds (last bits) - at both separations, also when the last wave is partly idle and when
    there are fewer particles than a wave."""
    import ctypes as C
    import sph_code_amd.ics as ics
    from sph_code_amd import _lib
    from scipy.spatial import cKDTree
    st = ics.WORKLOADS[workload](n, light=True)
    p = np.ascontiguousarray(st["points"]); m = np.ascontiguousarray(st["mass"])
    k = min(40, n)
    h = np.ascontiguousarray(cKDTree(p).query(p, k=k)[0][:, -1])
    dp = lambda a: a.ctypes.data_as(_lib.c_double_p)

    def run(per_thread, ws, order):
        if per_thread:
            monkeypatch.setenv("SPHX_GRAV_KERNEL", "0")
        else:
            monkeypatch.delenv("SPHX_GRAV_KERNEL", raising=False)
        c = _lib.Context()
        c.check(c.lib.sphx_set_gravity_order(c.h, order))
        out = np.empty((n, 3))
        c.check(c.lib.sphx_gravity_tree(c.h, n, dp(m), dp(p), dp(h), 0.0, 6.67430e-11, ws, 40, dp(out)))
        return out

    for ws, order in ((1, 1), (2, 1), (1, 2), (2, 2)):
        a, b = run(True, ws, order), run(False, ws, order)
        assert np.isfinite(a).all() and np.abs(a).max() > 0
        assert np.abs(a - b).max() <= 1e-13 * np.abs(a).max(), (ws, order, np.abs(a - b).max() / np.abs(a).max())
