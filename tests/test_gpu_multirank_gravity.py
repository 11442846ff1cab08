"""GPU tests of self-gravity in the decomposed step (multigpu.DistributedSim(gravity=...) on LibBackend: sphx_dev_gravity_*
and the gravity term of the sphx_dev_integrate* updates), ranks sharing the one GPU of the test box over gloo."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT

pytestmark = pytest.mark.gpu
K = 40


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _Gbig():
    from oracle import sph_oracle as orc
    return 3e7 * orc.G_NEWTON          # the light test cloud would hardly feel its own gravity otherwise


def _worker(rank, world, port, n, nsteps, gravity, forms, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sph_code_amd.ics as ics
    from sph_code_amd import multigpu as mg
    state = ics.polytrope_sphere(n, light=True)
    mine, lo, hi = mg.decompose_state(state, world, rank)
    kw = dict(forms="loop", d=ics.loop_d(state, K)) if forms == "loop" else {}
    sim = mg.DistributedSim(mine, lo, hi, mg.LibBackend(0, k=K), rank, world, device="cuda:0", comm_device="cpu",
                            gravity=gravity, G=_Gbig(), **kw)
    for _ in range(nsteps):
        sim.step()
    res = sim.owned_numpy()
    res["grav"] = np.array([sim.stats.get("grav_cells", 0), sim.stats.get("grav_parts", 0), sim.stats["redo"]])
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **res)
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()


def _run(world, n, nsteps, gravity, forms, tmp_path):
    mp.spawn(_worker, args=(world, _free_port(), n, nsteps, gravity, forms, str(tmp_path)), nprocs=world, join=True)
    parts = [dict(np.load(os.path.join(str(tmp_path), "rank%d.npz" % r))) for r in range(world)]
    gid = np.concatenate([p["gid"] for p in parts])
    assert np.array_equal(np.sort(gid), np.arange(n)), "particles lost or duplicated"
    order = np.argsort(gid)
    got = {k_: np.concatenate([p[k_] for p in parts])[order] for k_ in ("points", "velocities", "total_accel")}
    return got, parts


@pytest.mark.parametrize("forms", ["hydro_update", "loop"])
def test_two_ranks_direct_gravity_match_oracle(forms, tmp_path):
    """gravity="direct", world 2, polytrope_sphere(3000), 6 steps: x, v and total_accel within 1e-9 of their maxima of
    the oracle's step with gravity (loop forms: the oracle's loop-form step handed the direct sum at eps = median(h))."""
    from oracle import sph_oracle as orc
    import sph_code_amd.ics as ics
    n, nsteps = 3000, 6
    got, parts = _run(2, n, nsteps, "direct", forms, tmp_path)
    ref = ics.polytrope_sphere(n, light=True)
    d = ics.loop_d(ref, K) if forms == "loop" else None
    for it in range(nsteps):
        if forms == "loop":
            p, _ = orc.clamp_state(ref["points"], ref["velocities"])
            g = orc.gravity_direct(p, ref["mass"], np.median(orc.neighbors(p, np.inf, K, 0.0)[4]), G=_Gbig())
            ref = orc.step_loop(ref, d, n_neigh=K, eps=0.0, first=(it == 0), grav_accel=g)
        else:
            ref = orc.step(ref, n_neigh=K, eps=0.0, first=(it == 0), with_gravity=True, grav_G=_Gbig())
    for k_ in ("points", "velocities", "total_accel"):
        scale = np.max(np.abs(ref[k_]))
        err = np.max(np.abs(got[k_] - ref[k_]))
        print("%s %s: %.3g of the max" % (forms, k_, err / scale))
        assert err <= 1e-9 * scale, (k_, err / scale)
    for p in parts:                    # everything travelled as particles
        assert p["grav"][0] == 0 and p["grav"][1] >= nsteps * 0.4 * n


_fused = {}


def _fused_runs():
    """three steps of polytrope_sphere(20000) on the fused single-GPU loop: direct-sum gravity, and none"""
    if not _fused:
        import sph_code_amd.ics as ics
        from sph_code_amd.sim import Simulation
        s0 = ics.polytrope_sphere(20000, light=True)
        for key, kw in (("direct", dict(gravity="direct", G=_Gbig())), ("none", {})):
            sim = Simulation(s0, n_neigh=K, **kw)
            sim.step(3)
            _fused[key] = sim.download()["total_accel"].copy()
            sim.ctx.close()
    return _fused


@pytest.mark.parametrize("world", [2, 4])
def test_ranks_tree_gravity_tracks_direct(world, tmp_path):
    """gravity="tree", polytrope_sphere(20000), 3 steps: the rms of total_accel against the fused step with direct-sum
    gravity below 1e-2 of the rms of what gravity adds, which is above 0.1 of the gravity-free acceleration."""
    got, parts = _run(world, 20000, 3, "tree", "hydro_update", tmp_path)
    f = _fused_runs()
    grav = f["direct"] - f["none"]
    rms = lambda a: np.sqrt(np.mean(np.sum(a ** 2, axis=1)))
    assert rms(grav) > 0.1 * rms(f["none"])
    diff = rms(got["total_accel"] - f["direct"])
    print("world %d: rms difference %.3g of what gravity adds; exported per rank (cells, particles, redos): %s"
          % (world, diff / rms(grav), [p["grav"].tolist() for p in parts]))
    assert diff < 1e-2 * rms(grav)
    for p in parts:                    # cells did travel, and fewer particles than a rank holds per step and peer
        assert p["grav"][0] > 0


def test_one_rank_without_gravity_is_unchanged():
    """World 1, gravity=None: the state after 3 steps is bit-identical to a DistributedSim built without the new
    keywords, and equals the fused step as test_one_rank_device_api_matches_fused_step holds it."""
    import sph_code_amd.ics as ics
    from sph_code_amd import multigpu as mg
    from sph_code_amd.sim import Simulation
    n, nsteps = 20000, 3
    state = ics.polytrope_sphere(n, light=True)
    mine, lo, hi = mg.decompose_state(state, 1, 0)
    a = mg.DistributedSim(mine, lo, hi, mg.LibBackend(0, k=K), 0, 1, device="cuda:0")
    b = mg.DistributedSim(mine, lo, hi, mg.LibBackend(0, k=K), 0, 1, device="cuda:0", gravity=None, G=1.0, gravity_ws=2,
                          gravity_order=1, gravity_softening=3.0)
    sim = Simulation(state, n_neigh=K)
    for _ in range(nsteps):
        a.step(); b.step(); sim.step(1)
    ra, rb, rf = a.owned_numpy(), b.owned_numpy(), sim.download()
    for key in ("gid", "points", "velocities", "total_accel", "E_internal", "T", "sizes", "densities"):
        assert np.array_equal(ra[key], rb[key]), key
    order = np.argsort(rb["gid"])
    assert rf["dt"] == pytest.approx(rb["dt"], rel=1e-15)
    for key in ("points", "velocities", "total_accel", "E_internal", "T", "sizes", "densities"):
        np.testing.assert_allclose(rb[key][order], rf[key], rtol=1e-13, atol=0, err_msg=key)
    torch.cuda.synchronize()


def test_one_rank_tree_gravity_is_the_fused_tree_step():
    """World 1, gravity="tree": no peer, so the step is the fused step with tree gravity up to the frame the cells'
    centres are held in (the run's reference point against the fused step's own)."""
    import sph_code_amd.ics as ics
    from sph_code_amd import multigpu as mg
    from sph_code_amd.sim import Simulation
    n, nsteps = 20000, 3
    state = ics.polytrope_sphere(n, light=True)
    mine, lo, hi = mg.decompose_state(state, 1, 0)
    dsim = mg.DistributedSim(mine, lo, hi, mg.LibBackend(0, k=K), 0, 1, device="cuda:0", gravity="tree", G=_Gbig())
    sim = Simulation(state, n_neigh=K, gravity="tree", G=_Gbig())
    for _ in range(nsteps):
        dsim.step(); sim.step(1)
    a, b = sim.download(), dsim.owned_numpy()
    order = np.argsort(b["gid"])
    for key in ("points", "velocities", "total_accel"):
        np.testing.assert_allclose(b[key][order], a[key], rtol=0, atol=1e-10 * np.max(np.abs(a[key])), err_msg=key)
    assert "gravity" in dsim.host_ms and "gravity_eps" in dsim.host_ms
    torch.cuda.synchronize()
