#!/usr/bin/env python3
"""Rate of the arbitrary-point samplers (include/sphx.h sphx_state_sample) on the flagship cloud.

The N-particle polytrope after one step; two query sets - a 1024 x 1024 slice through the centre and 10^6 random points
in the bounding box - each sampled for the five fields in one call.  One warm-up call, then --repeats calls.  Every
call is timed twice: by the library's HIP events on its stream (sphx_arb_last_timing: points going up | reductions,
grid build, query sort, records | the sum and gate kernels | fields coming back), and by the host clock around the whole
synchronous call (what a caller waits for: the above plus argument handling and freshly allocated output pages).
Medians are reported; pairs per second is pair evaluations over the KERNEL time.

Culling: for each timed set, pair evaluations over contributing pairs (pairs with r < the particle's support, counted
on the host with a k-d tree; exact when all supports are equal, as in this all-gas equal-mass cloud, else an upper
bound of the contributing pairs from the largest support).  The NumPy restatement tests/arb_oracle.py is timed on 10^4
of the random points (the yardstick, not the code under test; it is handed the ball of the largest support, which
holds every contributing pair - the full ball of R = max(sizes) would not fit in memory) and its answers checked
against the library's on those points where that smaller ball passes the gate.  Prints one JSON line; --out FILE.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FIELDS = ("density", "dust_density", "temperature", "dust_temperature", "photoionization")


def timed(sim, q, d, n_part, value, repeats):
    sim.sample(q, d, fields=FIELDS, n_part=n_part, value=value, with_stats=True)          # warm-up: buffers, sort scratch
    host, dev = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        sim.sample(q, d, fields=FIELDS, n_part=n_part, value=value, with_stats=False)
        host.append((time.perf_counter() - t0) * 1e3)
        dev.append(sim.sample_timing())
    cand = sim.sample(q, d, fields=FIELDS, n_part=n_part, value=value, with_stats=True)["candidates"]
    med = {k: float(np.median([t[k] for t in dev])) for k in dev[0]}
    device_ms = sum(med.values())
    m = int(np.prod(q.shape[:-1]))
    return dict(points=m, ms_device=device_ms, ms_upload=med["upload"], ms_build=med["build"], ms_kernels=med["kernels"],
                ms_download=med["download"], ms_host_call=float(np.median(host)), ms_host_min=float(np.min(host)),
                ms_host_max=float(np.max(host)), points_per_s=m / (device_ms * 1e-3), candidates=int(cand),
                pairs_per_s_kernels=cand / (med["kernels"] * 1e-3))


def contributing_pairs(tree, q, sup):
    """pairs (point, particle) with r < the particle's support; exact for equal supports, else an upper bound."""
    lens = tree.query_ball_point(q.reshape(-1, 3), float(sup.max()) * (1.0 - 1e-15), p=2, eps=0, return_length=True,
                                 workers=-1)
    return int(np.sum(lens)), bool(sup.min() == sup.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--slice", type=int, default=1024)
    ap.add_argument("--random", type=int, default=1000000)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--cpu-points", type=int, default=10000, help="random points the host restatement evaluates")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import arb_oracle
    import sph_code_amd.compat as nsc
    from scipy.spatial import cKDTree
    from sph_code_amd import ics
    from sph_code_amd.sim import Simulation

    s = ics.polytrope_sphere(a.n, light=True, size_scale=ics.bench_size_scale(a.n))
    d = ics.loop_d(s, 40)
    rs = np.random.RandomState(1)
    n_part, value = 10.0 ** rs.uniform(50.0, 54.0, a.n), 10.0 ** rs.uniform(-12.0, -8.0, a.n)
    sim = Simulation(s, n_neigh=40)
    sim.step(1)
    st = sim.download()
    lo, hi = st["points"].min(axis=0), st["points"].max(axis=0)
    mid = 0.5 * (lo + hi)
    q_slice = ics.slice_points(mid, 2, (hi - lo)[:2], (a.slice, a.slice))
    q_rand = np.ascontiguousarray(lo + rs.rand(a.random, 3) * (hi - lo))
    res = dict(tool="arb_rate", n=a.n, repeats=a.repeats, d=d, radius=float(np.max(st["sizes"])),
               build=sim.ctx.build_info()["library"])
    res["slice"] = timed(sim, q_slice, d, n_part, value, a.repeats)
    res["random"] = timed(sim, q_rand, d, n_part, value, a.repeats)
    h = np.cbrt(s["mass"] / nsc.m_0) * d
    sup = np.where(s["particle_type"] == 0, h, np.where(s["particle_type"] == 2, st["sizes"], 0.0))
    tree = cKDTree(st["points"])
    for name, q in (("slice", q_slice), ("random", q_rand)):
        pairs, exact = contributing_pairs(tree, q, sup)
        res[name].update(contributing_pairs=pairs, contributing_pairs_exact=exact,
                         candidates_per_contributing=res[name]["candidates"] / max(pairs, 1))
    # the CPU figure: the restatement on 10^4 of the random points
    sub = np.ascontiguousarray(q_rand[:: max(1, len(q_rand) // a.cpu_points)][:a.cpu_points])
    gp = sim.sample(sub, d, fields=FIELDS, n_part=n_part, value=value, with_stats=True)
    kw = dict(points=st["points"], mass=s["mass"], particle_type=s["particle_type"], sizes=st["sizes"], T=st["T"],
              n_part=n_part, value=value, d=d, m_0=nsc.m_0)
    t0 = time.perf_counter()
    rows = tree.query_ball_point(sub, float(sup.max()), p=2, eps=0)
    rsr, mem = arb_oracle.to_csr(rows)
    o = arb_oracle.fields(arb_points=sub, row_start=rsr, members=mem, **kw)
    cpu_s = time.perf_counter() - t0
    same_gate = o["count"] > 1                       # (there the smaller ball decides as R's does: both pass)
    worst = 0.0
    for f in FIELDS:
        x, r, b = gp[f][same_gate], o[f][same_gate], o[f + "_bound"][same_gate]
        ok = np.isfinite(r) & np.isfinite(x)
        if ok.any():
            worst = max(worst, float(np.max(np.abs(x[ok] - r[ok]) / np.maximum(b[ok], 1e-300))))
    res["cpu"] = dict(points=len(sub), restatement_s=cpu_s, points_per_s=len(sub) / cpu_s,
                      points_checked=int(same_gate.sum()), worst_error_over_bound=worst)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
