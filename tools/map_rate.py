#!/usr/bin/env python3
"""Cost of the picture of the cloud (code_running.py:563-597) on the 1e6 polytrope and on the two-phase cube:
Simulation.project on the resident state in the driver's window - axes (1, 2), centre 0, half-width
sqrt(max_dist 11 / 9) with max_dist and d from length_scale(apply=False) - at 256 x 256 and 1024 x 1024 pixels, against
the floor of every host route, download() (unchanged by the projection: the parent build's time).

Per workload and image, over --repeats calls behind a warm-up: device ms per stage (footprints | count_scan | list_build |
tiles | read_back), the host clock of the call, pairs (the (particle, tile) list entries), pair evaluations (256 per
entry) per second of the tile kernel, and the tile kernel against the fp64 issue bound: every pair costs the seven fp64
operations of s = R^2 - ((u - x_u)^2 + (v - x_v)^2) and its test, each holding a SIMD's 16 lanes for 4 cycles per wave
(tools/fp64rate.hip, profiles/r03_valu_rates.txt), so the bound is evaluations x 7 / (CUs x 4 SIMDs x 16 lanes x clock).
The pairs inside a support pay the term on top; the ratio says how far the kernel is from the floor of the test alone.
The images of every repeat must agree bit for bit.  A refused call (more than 2^31 - 1 pairs) is recorded as such.

Prints one JSON line; --out FILE (meant for profiles/latest_map_profile.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPS_PER_PAIR = 7


def spread(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def device_rate():
    """fp64 lane-operations per second the device issues: CUs x 4 SIMDs x 16 lanes x clock."""
    import torch
    p = torch.cuda.get_device_properties(0)
    clock = float(getattr(p, "clock_rate", 2400000)) * 1e3
    return dict(cus=int(p.multi_processor_count), clock_hz=clock, lane_ops_per_s=p.multi_processor_count * 4 * 16 * clock)


def run(name, s, a, Simulation, rate):
    sim = Simulation(dict(s), n_neigh=a.k)
    sim.step(2)
    sim.ctx.check(sim.ctx.lib.sphx_sync(sim.ctx.h))
    ls = sim.length_scale(a.k, 8.0, apply=False)
    hw = float(np.sqrt(ls["max_dist"] * 11 / 9))
    res = dict(n=int(sim.n), d=ls["d"], half_width=hw, images={})
    dl = []
    for it in range(a.repeats + 1):
        t0 = time.perf_counter()
        sim.download()
        if it:
            dl.append((time.perf_counter() - t0) * 1e3)
    res["download_ms_host"] = spread(dl)
    for npix in a.npix:
        dev, host, outs, info = [], [], [], None
        try:
            for it in range(a.repeats + 1):
                t0 = time.perf_counter()
                m = sim.project(hw, npix, d=ls["d"])
                dt = (time.perf_counter() - t0) * 1e3
                if it:
                    host.append(dt); dev.append(sim.map_timing())
                    outs.append([m[f].tobytes() for f in ("gas_column", "dust_column", "gas_temperature", "dust_temperature", "count")])
                info = dict(pairs=m["pairs"], skipped=m["skipped"], count_max=int(m["count"].max()),
                            gas_column_max=float(m["gas_column"].max()), pixels_covered=int(np.count_nonzero(m["count"])))
        except (RuntimeError, ValueError) as e:
            res["images"]["%dx%d" % (npix, npix)] = dict(refused=str(e))
            continue
        ms = {k_: float(np.median([t[k_] for t in dev])) for k_ in dev[0]}
        evals = 256.0 * info["pairs"]
        bound_ms = evals * OPS_PER_PAIR / rate["lane_ops_per_s"] * 1e3
        info.update(device_ms=ms, device_ms_total=spread([sum(t.values()) for t in dev]), ms_host_call=spread(host),
                    pair_evaluations=evals, pair_evaluations_per_s=evals / (ms["tiles"] * 1e-3) if ms["tiles"] > 0 else None,
                    fp64_issue_bound_ms=bound_ms, tiles_over_bound=ms["tiles"] / bound_ms if bound_ms > 0 else None,
                    same_every_repeat=all(o == outs[0] for o in outs))
        res["images"]["%dx%d" % (npix, npix)] = info
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--k", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--npix", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import sph_code_amd.compat as nsc
    from sph_code_amd import ics
    from sph_code_amd.sim import Simulation

    rate = device_rate()
    scale = ics.bench_size_scale(a.n)
    res = dict(tool="map_rate", n=a.n, k=a.k, repeats=a.repeats, ops_per_pair=OPS_PER_PAIR, device=rate,
               build=nsc.context().build_info()["library"])
    res["polytrope"] = run("polytrope", ics.polytrope_sphere(a.n, size_scale=scale), a, Simulation, rate)
    res["two_phase"] = run("two_phase", ics.two_phase(a.n, size_scale=scale), a, Simulation, rate)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
