"""Self-gravity in the decomposed step (multigpu.DistributedSim(gravity=...)) over gloo on the CPU: the protocol - boxes,
softening from every rank's h, export counts, the two record exchanges, the term handed to each of the update's entry
points, snapshot and restart - with a test-only EXACT backend whose export is "all owned particles" and whose local and
remote sums are pieces of the oracle's direct sum, against the oracle's step with gravity."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT
from test_multigpu_cpu import OracleBackend, OracleFusedBackend, _free_port

K = 16
N, NSTEPS = 3000, 6


def _gravity_mixin(base):
    class ExactGravity(base):
        """base + gravity: every owned particle travels to every peer that owns any; sums by orc.gravity_direct."""

        def gravity_build(self, pos, m, n_owned, ref):
            self.gp, self.gm = pos.numpy()[:n_owned].copy(), m.numpy()[:n_owned].copy()

        def gravity_local(self, ws, G, eps):
            return torch.from_numpy(self.orc.gravity_direct(self.gp, self.gm, float(eps), G=G))

        def gravity_export(self, boxes, rank, ws, cap_cells, cap_parts):
            b = boxes.numpy()
            world = len(b)
            rec = np.concatenate([self.gp, self.gm[:, None]], axis=1)
            counts = np.zeros((world, 2), np.int32)
            out = []
            for q in range(world):
                if q != rank and (b[q, 3:] >= b[q, :3]).all():
                    counts[q, 1] = len(rec)
                    out.append(rec)
            parts = np.concatenate(out) if out else np.zeros((0, 4))
            buf = np.full((max(cap_parts, 1), 4), np.nan)                  # (nothing beyond the capacity)
            keep = min(len(parts), cap_parts)
            buf[:keep] = parts[:keep]
            return torch.zeros((max(cap_cells, 1), 12), dtype=torch.float64), torch.from_numpy(buf), torch.from_numpy(counts)

        def gravity_remote(self, pos_owned, cells, parts, G, eps, accel):
            assert cells.shape[0] == 0
            t, src = pos_owned.numpy(), parts.numpy()
            assert np.isfinite(src).all()
            nt = len(t)
            a = self.orc.gravity_direct(np.vstack([t, src[:, :3]]), np.append(np.zeros(nt), src[:, 3]), float(eps), G=G)
            accel += torch.from_numpy(a[:nt])

        def set_gravity_accel(self, grav):
            self.gacc = None if grav is None else grav.numpy().copy()

        def _take_grav(self, no):
            g, self.gacc = getattr(self, "gacc", None), None
            return None if g is None else g[:no]

        def integrate(self, no, pos, vel, acc, E, T, m, mu, gam, ptype, ha, va, vh, dt):
            n = lambda t: t.numpy()[:no]
            drag = getattr(self, "terms", None)
            self.terms = None
            p, v, tot, En, Tn = self.orc.integrate(n(pos), n(vel), n(acc), n(E), n(m), n(mu), n(gam), n(ptype),
                                                   n(ha), n(va), n(vh), dt, self._take_grav(no), drag)
            for dst, src in ((pos, p), (vel, v), (acc, tot), (E, En), (T, Tn)):
                dst[:no] = torch.from_numpy(np.ascontiguousarray(src))

        def integrate_loop(self, no, pos, vel, acc, E, T, m, mu, gam, ptype, delp, rho, va, vh, dt, red2=None, first=False,
                           fixed_dt=0.0):
            grav = self._take_grav(no)
            if red2 is not None:
                if float(red2[0]) > 0.5:
                    return torch.zeros(1, dtype=torch.float64)
                dt = self._dt(red2, first, fixed_dt)
            o = self.orc
            n = lambda t: t.numpy()[:no]
            pa, visc = o.assemble_loop(n(delp), n(rho), None, n(ptype), n(va), None)
            p, v, tot, En, Tn = o.leapfrog(n(pos), n(vel), n(acc), n(E), n(m), n(mu), n(gam), pa, visc, n(vh), dt, grav)
            for dst, src in ((pos, p), (vel, v), (acc, tot), (E, En), (T, Tn)):
                dst[:no] = torch.from_numpy(np.ascontiguousarray(src))
            return torch.tensor([dt], dtype=torch.float64) if red2 is not None else None

    return ExactGravity


def _G():
    from oracle import sph_oracle as orc
    return 3e7 * orc.G_NEWTON


def _worker(rank, world, port, fused, forms, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sph_code_amd.ics as ics
    from sph_code_amd import multigpu as mg
    state = ics.polytrope_sphere(N, light=True)
    mine, lo, hi = mg.decompose_state(state, world, rank)
    Backend = _gravity_mixin(OracleFusedBackend if fused else OracleBackend)
    kw = dict(gravity="direct", G=_G(), migrate_every=1, forms=forms)
    if forms == "loop":
        kw["d"] = ics.loop_d(state, K)
    sim = mg.DistributedSim(mine, lo, hi, Backend(K), rank, world, device="cpu", **kw)
    prefix = os.path.join(out_dir, "snap")
    for it in range(NSTEPS):
        if it == NSTEPS // 2:
            sim.snapshot(prefix)
        sim.step()
    res = sim.owned_numpy()
    res["grav"] = np.array([sim.stats.get("grav_cells", 0), sim.stats.get("grav_parts", 0), sim.stats["migrated"],
                            sim.host_ms.get("gravity", 0.0), sim.host_ms.get("gravity_eps", 0.0)])
    # the run resumed from the snapshot: the same bits as the uninterrupted one
    again = mg.DistributedSim.from_snapshot(prefix, Backend(K), rank, world, device="cpu", migrate_every=1)
    assert again.gravity == "direct" and again.grav_G == _G() and again.gravity_ws == 1 and again.gravity_order == 2
    assert again.gravity_softening is None and again.grav_ref == sim.grav_ref
    for it in range(NSTEPS // 2, NSTEPS):
        again.step()
    r2 = again.owned_numpy()
    same = all(np.array_equal(res[k_], r2[k_]) for k_ in ("gid", "points", "velocities", "total_accel", "E_internal", "T"))
    res["restart_same_bits"] = np.int64(1 if same else 0)
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **res)
    dist.barrier()
    dist.destroy_process_group()


def _run(world, fused, forms, tmp_path):
    mp.spawn(_worker, args=(world, _free_port(), fused, forms, str(tmp_path)), nprocs=world, join=True)
    parts = [dict(np.load(os.path.join(str(tmp_path), "rank%d.npz" % r))) for r in range(world)]
    gid = np.concatenate([p["gid"] for p in parts])
    assert np.array_equal(np.sort(gid), np.arange(N)), "particles lost or duplicated"
    order = np.argsort(gid)
    got = {k_: np.concatenate([p[k_] for p in parts])[order] for k_ in ("points", "velocities", "total_accel")}
    return got, parts


_ref_cache = {}


def _reference(forms):
    """the oracle's six steps with gravity (computed once per form and left unchanged)"""
    if forms not in _ref_cache:
        from oracle import sph_oracle as orc
        import sph_code_amd.ics as ics
        s = ics.polytrope_sphere(N, light=True)
        d = ics.loop_d(s, K) if forms == "loop" else None
        for it in range(NSTEPS):
            if forms == "loop":
                p, _ = orc.clamp_state(s["points"], s["velocities"])
                h = orc.neighbors(p, np.inf, K, 0.0)[4]
                g = orc.gravity_direct(p, s["mass"], np.median(h), G=_G())
                s = orc.step_loop(s, d, n_neigh=K, eps=0.0, first=(it == 0), grav_accel=g)
            else:
                s = orc.step(s, n_neigh=K, eps=0.0, first=(it == 0), with_gravity=True, grav_G=_G())
        _ref_cache[forms] = s
    return _ref_cache[forms]


def _check(got, parts, ref, world):
    for k_ in ("points", "velocities", "total_accel"):
        scale = np.max(np.abs(ref[k_]))
        err = np.max(np.abs(got[k_] - ref[k_]))
        assert err <= 1e-9 * scale, (k_, err / scale)
    for p in parts:
        assert int(p["restart_same_bits"]) == 1
        cells, sent = p["grav"][0], p["grav"][1]
        # the redo loop may run a step's gravity more than once; each run sends every owned particle to every peer
        assert cells == 0 and sent >= NSTEPS * (world - 1) * 0.5 * N / world
        assert p["grav"][3] > 0.0 and p["grav"][4] > 0.0                 # host_ms["gravity"], ["gravity_eps"]


@pytest.mark.parametrize("world,fused", [(2, False), (2, True), (4, True)])
def test_gloo_gravity_matches_oracle_step_and_restarts(world, fused, tmp_path):
    """6 steps of polytrope_sphere(3000) with G = 3e7 G_NEWTON, migration on every replan, world 2 (the plain update and
    the update that takes verdict and dt from device memory) and world 4: x, v and total_accel within 1e-9 of their
    maxima of the oracle's step with gravity; the run resumed from a snapshot taken half way gives the same bits."""
    got, parts = _run(world, fused, "hydro_update", tmp_path)
    ref = _reference("hydro_update")
    _check(got, parts, ref, world)
    # gravity really is in the acceleration
    from oracle import sph_oracle as orc
    import sph_code_amd.ics as ics
    s = ics.polytrope_sphere(N, light=True)
    for it in range(NSTEPS):
        s = orc.step(s, n_neigh=K, eps=0.0, first=(it == 0))
    assert np.max(np.abs(ref["total_accel"] - s["total_accel"])) > 1e-3 * np.max(np.abs(ref["total_accel"]))


def test_gloo_gravity_in_loop_form_steps(tmp_path):
    """The same through the loop forms' update (sphx_dev_integrate_loop's counterpart), world 2, against the oracle's
    loop-form step handed the direct sum at eps = median(h) of each step."""
    got, parts = _run(2, True, "loop", tmp_path)
    _check(got, parts, _reference("loop"), 2)


def test_gravity_needs_a_backend_with_the_methods_and_sane_settings():
    import sph_code_amd.ics as ics
    from sph_code_amd import multigpu as mg
    state = ics.polytrope_sphere(200, light=True)
    mine, lo, hi = mg.decompose_state(state, 1, 0)
    with pytest.raises(ValueError, match="gravity_build"):
        mg.DistributedSim(mine, lo, hi, OracleBackend(K), 0, 1, device="cpu", gravity="direct")
    Backend = _gravity_mixin(OracleBackend)
    for bad in (dict(gravity="fmm"), dict(gravity="tree", gravity_ws=0), dict(gravity="tree", gravity_order=3),
                dict(gravity="direct", gravity_softening=-1.0)):
        with pytest.raises(ValueError):
            mg.DistributedSim(mine, lo, hi, Backend(K), 0, 1, device="cpu", **bad)
    # one rank, a fixed softening: the oracle's direct sum at that eps, no exchange
    sim = mg.DistributedSim(mine, lo, hi, Backend(K), 0, 1, device="cpu", gravity="direct", G=_G(), gravity_softening=1e15)
    sim.step()
    assert "gravity" in sim.host_ms and "gravity_eps" not in sim.host_ms
