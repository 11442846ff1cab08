"""GPU tests (-m gpu) of the pairwise artificial viscosity (visc_mode="pairwise"): the array API against the NumPy
restatement of tests/test_pairwise_cpu.py, trajectories against an oracle step composed with it, the pass forms bit for
bit, live physics where the axis-0 mode loses its viscosity, the device-pointer path and the C ABI's argument checks."""
import numpy as np
import pytest

from conftest import GOLDEN_CASES, hydro_args, load_golden
from test_gpu_parity import VARIANT_CASES, VARIANT_IDS
from test_pairwise_cpu import signed_close, viscosity_sums

pytestmark = pytest.mark.gpu
SPHX_E_ARG = -1                # include/sphx.h


@pytest.fixture(scope="module")
def nsc():
    import sph_code_amd.compat as nsc_mod
    nsc_mod.context()
    return nsc_mod


@pytest.mark.parametrize("case", GOLDEN_CASES)
@pytest.mark.parametrize("clip_grad", [False, True])
def test_hydro_update_pairwise_vs_restatement(nsc, case, clip_grad):
    args = hydro_args(load_golden(case))
    out = nsc.hydro_update(*args, clip_grad=clip_grad, visc_mode="pairwise")
    axis0 = nsc.hydro_update(*args, clip_grad=clip_grad)
    ref, _ = viscosity_sums(args, clip_grad=clip_grad)
    signed_close(out[1], ref[1], "visc_accel")
    signed_close(out[2], ref[2], "visc_heat")
    assert (out[2] >= 0).all()
    for i in (0, 3, 4, 5, 6):                   # density, number density, hydro_accel, species, dust: untouched
        assert np.array_equal(out[i], axis0[i], equal_nan=True), i
    assert not np.array_equal(out[1], axis0[1])


def _oracle_step_pairwise(s, K, first, fixed_dt=0.0, clip_grad=False):
    from oracle import sph_oracle as orc
    s = dict(s)
    p, v = orc.clamp_state(s["points"], s["velocities"])
    nb, _, _, _, h = orc.neighbors(p, np.inf, K, eps=0.0)
    ct = orc.crossing_time(nb, v, h, s["particle_type"])
    dt = fixed_dt if fixed_dt > 0 else orc.timestep(ct, first)
    n = len(p)
    args = (nb, p, s["mass"], h, np.ones((n, 1)), s["particle_type"], s["T"], s["mu_array"], s["gamma_array"], v)
    (ha, va, vh, rho, nden, _, _), _ = viscosity_sums(args, clip_grad=clip_grad)
    p, v, total, E, T = orc.integrate(p, v, s["total_accel"], s["E_internal"], s["mass"], s["mu_array"],
                                      s["gamma_array"], s["particle_type"], ha, va, vh, dt)
    s.update(points=p, velocities=v, total_accel=total, E_internal=E, T=T, dt=dt, sizes=h, densities=rho,
             visc_heat=vh)
    return s


@pytest.mark.parametrize("clip_grad", [False, True])
@pytest.mark.parametrize("workload", ["uniform_sphere", "sedov", "polytrope"])
def test_pairwise_step_trajectory_vs_oracle(workload, clip_grad):
    import sph_code_amd.ics as ics
    from sph_code_amd.sim import Simulation
    n, K, nsteps = (10000 if workload == "uniform_sphere" else 4096), 40, 10
    s0 = ics.WORKLOADS[workload](n)
    fixed_dt = ics.cfl_dt(s0, K) if workload == "sedov" else 0.0
    sim = Simulation(s0, n_neigh=K, clip_grad=clip_grad, visc_mode="pairwise")
    ref = dict(s0)
    for it in range(nsteps):
        sim.step(1, fixed_dt=fixed_dt)
        ref = _oracle_step_pairwise(ref, K, it == 0, fixed_dt, clip_grad)
        got = sim.download()
        assert got["dt"] == pytest.approx(ref["dt"], rel=1e-12), "dt at step %d" % it
        if it == 2:
            R0 = np.max(np.abs(s0["points"]))
            assert np.max(np.abs(got["points"] - ref["points"])) <= 1e-12 * R0
            assert np.max(np.abs(got["velocities"] - ref["velocities"])) <= 1e-10 * np.max(np.abs(ref["velocities"]))
    # (unclipped, the uniform sphere's neighbour-side gradient, growing as r^4, flings a few particles to inf by step 10 -
    #  in the oracle as on the device: the same particles, at most 1 % of them, the finite rest compared as
    #  test_step_trajectory_vs_oracle does; everywhere else nothing may be non-finite)
    n_lost = int((~np.isfinite(ref["points"]).all(axis=1)).sum())
    assert n_lost <= (0.01 * n if (workload == "uniform_sphere" and not clip_grad) else 0), n_lost
    signed_close(got["points"], ref["points"], "points", tol=1e-9)
    signed_close(got["velocities"], ref["velocities"], "velocities", tol=1e-9)
    np.testing.assert_allclose(got["sizes"], ref["sizes"], rtol=1e-9)
    np.testing.assert_allclose(got["densities"], ref["densities"], rtol=1e-9)
    np.testing.assert_allclose(got["E_internal"], ref["E_internal"], rtol=1e-9)
    np.testing.assert_allclose(got["T"], ref["T"], rtol=1e-9)


@pytest.mark.parametrize("workload,n,K,clip_grad,slots", VARIANT_CASES, ids=VARIANT_IDS)
def test_pairwise_step_variants_are_bit_identical(workload, n, K, clip_grad, slots, monkeypatch):
    """LDS pass (default), LDS with 300 image slots (global-memory fallback; test_gpu_parity.py's VARIANT_CASES say where
    fewer), gathers in blob order, gathers in storage order: one answer, bit for bit; no failure counter set."""
    import sph_code_amd.ics as ics
    from sph_code_amd.sim import Simulation
    s0 = ics.WORKLOADS[workload](n)
    res = {}
    for name, env in (("lds", {}), ("lds_overflow", {"SPHX_BLOB_SLOTS": str(slots)}), ("blob_gather", {"SPHX_LDS": "0"}),
                      ("storage_order", {"SPHX_BLOB": "0"})):
        for k_, v in env.items():
            monkeypatch.setenv(k_, v)
        sim = Simulation(s0, n_neigh=K, clip_grad=clip_grad, visc_mode="pairwise")
        sim.step(4)
        res[name] = sim.download()
        assert sim.failures() == dict.fromkeys(Simulation.FAILURE_COUNTERS, 0), (name, sim.failures())
        for k_ in env:
            monkeypatch.delenv(k_)
    for name in ("lds_overflow", "blob_gather", "storage_order"):
        for key in ("points", "velocities", "E_internal", "T", "sizes", "densities", "total_accel"):
            assert np.array_equal(res["lds"][key], res[name][key], equal_nan=True), (name, key)


@pytest.mark.timeout(600)
def test_pairwise_timed_step_path_equals_array_path_at_full_size(nsc):
    """Two steps of the 10^6 polytrope through the fused loop (LDS pass) equal, bit for bit, compat.neighbors ->
    compat.hydro_update(visc_mode="pairwise") (gather pass) -> sphx_dev_integrate; nothing for nan_to_num to hide."""
    import ctypes as C
    import torch
    import sph_code_amd.ics as ics
    from sph_code_amd import _lib
    from sph_code_amd.sim import Simulation
    n, K = 1_000_000, 40
    s = ics.polytrope_sphere(n)
    sim = Simulation(s, n_neigh=K, visc_mode="pairwise")
    ctx = _lib.Context(0)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
    P = lambda x: C.c_void_p(x.data_ptr())
    fu1 = np.ones((n, 1))
    tm, tmu, tgam, tpt = t(s["mass"]), t(s["mu_array"]), t(s["gamma_array"]), t(s["particle_type"])
    cur = dict(points=s["points"], velocities=s["velocities"], total_accel=np.zeros((n, 3)),
               E_internal=s["E_internal"], T=s["T"])
    for it in range(2):
        sim.step(1)
        got = sim.download()
        p, v = nsc.clamp_state(cur["points"], cur["velocities"])
        idx, _, d, nontriv, h = nsc.neighbors(p, np.inf, K)
        assert np.array_equal(got["sizes"], h), "h, step %d" % it
        ha, va, vh, rho, nden, F, rhod = nsc.hydro_update(idx, p, s["mass"], h, fu1, s["particle_type"], cur["T"],
                                                          s["mu_array"], s["gamma_array"], v, visc_mode="pairwise")
        assert np.array_equal(got["densities"], rho), "rho, step %d" % it
        assert np.array_equal(got["visc_heat"], vh), "visc_heat, step %d" % it
        assert (vh >= 0).all()
        ct = nsc.crossing_time(idx, v, h, s["particle_type"])
        assert got["dt"] == pytest.approx(nsc.timestep(ct, it == 0), rel=1e-12)
        pos, vel, acc, E = t(p), t(v), t(cur["total_accel"]), t(cur["E_internal"])
        T = torch.zeros_like(E)
        tha, tva, tvh = t(ha), t(va), t(vh)
        torch.cuda.synchronize()
        ctx.check(ctx.lib.sphx_dev_integrate(ctx.h, n, P(pos), P(vel), P(acc), P(E), P(T), P(tm), P(tmu), P(tgam),
                                             P(tpt), P(tha), P(tva), P(tvh), float(got["dt"])))
        ctx.check(ctx.lib.sphx_sync(ctx.h))
        cur = dict(points=pos.cpu().numpy(), velocities=vel.cpu().numpy(), total_accel=acc.cpu().numpy(),
                   E_internal=E.cpu().numpy(), T=T.cpu().numpy())
        for key in ("total_accel", "points", "velocities", "E_internal", "T"):
            assert np.array_equal(got[key], cur[key]), "%s, step %d" % (key, it)
    f = sim.failures()
    assert all(v_ == 0 for v_ in f.values()), f
    ctx.close()


def test_pairwise_viscosity_stays_live():
    """Where the axis-0 mode drives T below zero on a third of the uniform sphere in step 1 and loses every viscous
    force from step 2 on (test_failure_counters_say_what_nan_to_num_hid), the pairwise mode heats: T > 0 everywhere,
    no failure counter set; with clip_grad the polytrope runs 50 steps clean."""
    import sph_code_amd.ics as ics
    from sph_code_amd.sim import Simulation
    n = 3000
    base = ics.uniform_sphere(n)
    zero = dict.fromkeys(Simulation.FAILURE_COUNTERS, 0)
    sim = Simulation(base, n_neigh=40, visc_mode="pairwise")
    sim.ctx.set_timing_detail(True)
    sim.step(1)
    assert (sim.download()["T"] > 0).all()
    sim.step(1)
    assert sim.failures() == zero
    st = sim.stats()
    assert st["ms_pi"] == 0.0 and st["ms_visc"] > 0.0, st        # one fused pass
    sim = Simulation(ics.polytrope_sphere(20000), n_neigh=40, clip_grad=True, visc_mode="pairwise")
    sim.step(50)
    assert sim.failures() == zero


def test_pairwise_device_api_matches_fused_step():
    """One rank of DistributedSim(visc_mode="pairwise") through sphx_dev_visc_pairwise equals the fused pairwise step;
    the m Pi_j halo phase (backend.pi / backend.visc) is not run."""
    import sph_code_amd.ics as ics
    from sph_code_amd import multigpu as mg
    from sph_code_amd.sim import Simulation
    K, n, nsteps = 40, 20000, 4
    state = ics.polytrope_sphere(n, light=True)
    sim = Simulation(state, n_neigh=K, visc_mode="pairwise")
    mine, lo, hi = mg.decompose_state(state, 1, 0)
    be = mg.LibBackend(0, k=K, visc_mode="pairwise")

    def _no_pi(*a, **k):
        raise AssertionError("the Pi pass ran in pairwise mode")
    be.pi = be.visc = _no_pi
    dsim = mg.DistributedSim(mine, lo, hi, be, 0, 1, device="cuda:0")
    assert dsim.visc_mode == "pairwise"                 # (the backend's)
    for _ in range(nsteps):
        sim.step(1)
        dsim.step()
    a = sim.download()
    b = dsim.owned_numpy()
    order = np.argsort(b["gid"])
    assert a["dt"] == pytest.approx(b["dt"], rel=1e-15)
    for key in ("points", "velocities", "total_accel", "E_internal", "T", "sizes", "densities"):
        np.testing.assert_allclose(b[key][order], a[key], rtol=1e-13, atol=0, err_msg=key)


def test_pairwise_snapshot_carries_the_mode(tmp_path):
    import sph_code_amd.ics as ics
    from sph_code_amd import multigpu as mg
    state = ics.polytrope_sphere(5000, light=True)
    mine, lo, hi = mg.decompose_state(state, 1, 0)
    dsim = mg.DistributedSim(mine, lo, hi, mg.LibBackend(0, k=40, visc_mode="pairwise"), 0, 1, device="cuda:0",
                             visc_mode="pairwise")
    dsim.step()
    prefix = str(tmp_path / "snap")
    dsim.snapshot(prefix)
    with pytest.raises(ValueError):                     # the file says pairwise, the backend says ref_axis0
        mg.DistributedSim.from_snapshot(prefix, mg.LibBackend(0, k=40), 0, 1, device="cuda:0")
    back = mg.DistributedSim.from_snapshot(prefix, mg.LibBackend(0, k=40, visc_mode="pairwise"), 0, 1, device="cuda:0")
    assert back.visc_mode == "pairwise"
    f = prefix + ".rank0.npz"
    z = dict(np.load(f))
    del z["visc_mode"]
    np.savez(f, **z)
    old = mg.DistributedSim.from_snapshot(prefix, mg.LibBackend(0, k=40), 0, 1, device="cuda:0")
    assert old.visc_mode == "ref_axis0"


def test_pairwise_c_abi_argument_errors(nsc):
    import sph_code_amd.ics as ics
    from sph_code_amd import _lib
    from sph_code_amd._lib import dp
    from sph_code_amd.sim import Simulation
    g = load_golden("small_n256_k16")
    c = nsc.context()
    n, K = g["nb_idx"].shape
    nb = np.ascontiguousarray(g["nb_idx"], dtype=np.int64)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    out3, out1 = np.empty((n, 3)), np.empty(n)
    args = [f(g[k_]) for k_ in ("points", "mass", "nb_h")]
    rc = c.lib.sphx_hydro_update(c.h, n, K, 0, nb.ctypes.data_as(_lib.c_int64_p), dp(args[0]),
                                 dp(args[1]), dp(args[2]), None, dp(f(g["particle_type"])), dp(f(g["T"])),
                                 dp(f(g["mu_array"])), dp(f(g["gamma_array"])), dp(f(g["velocities"])), 2,
                                 dp(out3), None, None, None, None, None, None)
    assert rc == SPHX_E_ARG
    s0 = ics.uniform_sphere(2000)
    sim = Simulation(s0, n_neigh=40, forms="loop", d=ics.loop_d(s0, 40))
    assert sim.ctx.lib.sphx_set_visc_mode(sim.ctx.h, 1) == SPHX_E_ARG
    assert sim.ctx.lib.sphx_set_visc_mode(sim.ctx.h, 0) == 0
    assert c.lib.sphx_set_visc_mode(c.h, 2) == SPHX_E_ARG


def test_pairwise_device_pass_refuses_records_built_before_the_mode():
    """sphx_dev_visc_pairwise needs the pairwise factor the record build stores: records built in ref_axis0 mode are a
    state error, not a silently zero viscosity."""
    import torch
    import sph_code_amd.ics as ics
    from sph_code_amd import multigpu as mg
    state = ics.polytrope_sphere(5000, light=True)
    mine, lo, hi = mg.decompose_state(state, 1, 0)
    be = mg.LibBackend(0, k=40)
    dsim = mg.DistributedSim(mine, lo, hi, be, 0, 1, device="cuda:0")
    dsim.step()                                         # search + records in ref_axis0 mode
    be.set_visc_mode("pairwise")
    rho = torch.ones(be.n_total, dtype=torch.float64, device="cuda:0")
    with pytest.raises(Exception, match="pairwise"):
        be.visc_pairwise(rho, rho)
