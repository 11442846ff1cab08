"""GPU tests of the decomposed path in pairwise viscosity mode (DistributedSim / LibBackend visc_mode="pairwise",
sphx_dev_visc_pairwise): two ranks sharing the one GPU of the test box, with interior workgroups under the rho_j halo
phase and boundary ones after it, against the single-GPU fused pairwise step; and the overlap changes no bit."""
import os
import socket
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before libsphx.so: see tests/conftest.py)
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


def _worker(rank, world, port, n, nsteps, workload, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sph_code_amd.ics as ics
    from sph_code_amd import multigpu as mg
    state = ics.WORKLOADS[workload](n, light=True)
    mine, lo, hi = mg.decompose_state(state, world, rank)
    be = mg.LibBackend(0, k=K, visc_mode="pairwise")
    calls = {"pairwise": 0}

    def _no_pi(*a, **k):                 # pairwise: no Pi pass, hence no m Pi_j halo phase behind it
        raise AssertionError("the Pi pass ran in pairwise mode")
    be.pi = be.visc = _no_pi
    visc_pairwise = be.visc_pairwise

    def _counted(*a, **k):
        calls["pairwise"] += 1
        return visc_pairwise(*a, **k)
    be.visc_pairwise = _counted
    sim = mg.DistributedSim(mine, lo, hi, be, rank, world, device="cuda:0", comm_device="cpu", visc_mode="pairwise")
    for _ in range(nsteps):
        sim.step()
    res = sim.owned_numpy()
    res["blob_split"] = np.array(sim.backend.blob_split_counts())
    res["pairwise_calls"] = np.array(calls["pairwise"])
    res["steps_run"] = np.array(nsteps + sim.stats["redo"])
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **res)
    dist.barrier()
    dist.destroy_process_group()


def _gather(out_dir, world, keys):
    parts = [dict(np.load(os.path.join(str(out_dir), "rank%d.npz" % r))) for r in range(world)]
    order = np.argsort(np.concatenate([p["gid"] for p in parts]))
    got = {k_: np.concatenate([p[k_] for p in parts])[order] for k_ in keys}
    return parts, got


def test_two_ranks_pairwise_match_the_fused_step_at_2e5_particles(tmp_path):
    """Both kinds of workgroup on both ranks (the interior ones run sphx_dev_visc_pairwise before the ghosts' rho_j
    arrive, the boundary ones after: two calls per step), ghost records with their pairwise factor from the second
    record build, no Pi pass: against the single-GPU fused pairwise loop, with the tolerances of
    test_two_ranks_match_the_fused_step_at_2e5_particles."""
    import sph_code_amd.ics as ics
    from sph_code_amd.sim import Simulation
    n, nsteps, world = 200000, 4, 2
    mp.spawn(_worker, args=(world, _free_port(), n, nsteps, "polytrope", str(tmp_path)), nprocs=world, join=True)
    parts, got = _gather(tmp_path, world, ("points", "velocities", "total_accel", "E_internal", "sizes", "densities"))
    assert all(p["blob_split"][0] > 100 and p["blob_split"][1] > 20 for p in parts)
    assert all(int(p["pairwise_calls"]) == 2 * int(p["steps_run"]) for p in parts)     # interior + boundary, every step
    state = ics.WORKLOADS["polytrope"](n, light=True)
    sim = Simulation(state, n_neigh=K, visc_mode="pairwise")
    sim.step(nsteps)
    ref = sim.download()
    assert sim.failures() == dict.fromkeys(Simulation.FAILURE_COUNTERS, 0)
    assert float(parts[0]["dt"]) == pytest.approx(ref["dt"], rel=1e-13)
    np.testing.assert_allclose(got["sizes"], ref["sizes"], rtol=1e-13)
    np.testing.assert_allclose(got["densities"], ref["densities"], rtol=1e-12)
    np.testing.assert_allclose(got["E_internal"], ref["E_internal"], rtol=1e-11)
    for k_ in ("points", "velocities", "total_accel"):
        assert np.max(np.abs(got[k_] - ref[k_])) <= 1e-10 * np.max(np.abs(ref[k_])), k_


def test_two_ranks_pairwise_interior_blobs_under_the_halo_phase_change_nothing(tmp_path, monkeypatch):
    """SPHX_MG_OVERLAP on (interior workgroups under the rho_j phase) and off: the same bits."""
    n, nsteps, world = 20000, 5, 2
    keys = ("points", "velocities", "E_internal", "sizes", "densities", "total_accel")
    res = {}
    for ov in ("1", "0"):
        monkeypatch.setenv("SPHX_MG_OVERLAP", ov)
        out = tmp_path / ("ov" + ov)
        out.mkdir()
        mp.spawn(_worker, args=(world, _free_port(), n, nsteps, "polytrope", str(out)), nprocs=world, join=True)
        parts, res[ov] = _gather(out, world, keys)
        res[ov]["dt"] = float(parts[0]["dt"])
        if ov == "1":
            assert all(p["blob_split"][0] > 0 and p["blob_split"][1] > 0 for p in parts)
            assert all(int(p["pairwise_calls"]) == 2 * int(p["steps_run"]) for p in parts)
    assert res["1"]["dt"] == res["0"]["dt"]
    for k_ in keys:
        assert np.array_equal(res["1"][k_], res["0"][k_]), k_
