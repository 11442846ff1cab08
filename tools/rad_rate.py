#!/usr/bin/env python3
"""Rate of the radiative transfer (include/sphx.h sphx_state_rad_transfer) on the flagship cloud.

The N-particle polytrope after one step; --sources seeded particles stand for the selected stars (the state's own
particle types are kept: an all-gas cloud, every particle a non-star), --targets seeded particles for the sampled gas
(the reference's own sampling, N^0.35, gives 125 at 10^6).  One warm-up call, then --repeats calls, each timed by the
library's HIP events on its stream (sphx_rad_last_timing: inputs going up and prepared | columns | spread and deposit |
outputs coming back) and by the host clock around the whole synchronous call.  Medians are reported.

  ray_particle_per_s      n_src n_dst N evaluations of the column's pair term over the column time
  src_dst_particle_per_s  n_src n_dst N_gas terms of lum_factor's sum over the deposit time
each also as a share of the fp64 issue bound: 16 lanes per cycle per SIMD (profiles/r03_valu_rates.txt: a v_fma_f64
wave-instruction issues every ~4 cycles) x 4 SIMDs x the CUs x the clock, over the VALU instructions per evaluation.
Those come from the kernels' own disassembly (hipcc -S of sphx_rad.hip, built as build.py builds it): the VALU
instructions of the innermost loop over the evaluations one trip makes - one fp64 compare per pair in the line-mode column
loop, SPHX_RAD_SRC_CHUNK terms per reciprocal square root in the deposit loop.  Prints one JSON line; --out FILE.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLOCK_HZ = 2.1e9            # profiles/r03_valu_rates.txt: the clock the fp64 rate loops ran at
LANES_PER_CYCLE_PER_SIMD = 16


def loops_of(asm, kernel):
    """-> the innermost loops of `kernel` in hipcc's assembly listing, each a list of instruction lines."""
    lines = asm.split("\n")
    i0 = next(i for i, l in enumerate(lines) if re.match(re.escape(kernel) + r"\S*:", l))
    i1 = next(i for i in range(i0, len(lines)) if lines[i].strip().startswith(".Lfunc_end"))
    body = lines[i0:i1]
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
    spans = []
    for i, l in enumerate(body):
        m = re.search(r"s_cbranch_\w+\s+(\.LBB\d+_\d+)", l)
        if m and labels.get(m.group(1), len(body)) < i:
            spans.append((labels[m.group(1)], i))
    inner = [s for s in spans if not any(o != s and s[0] <= o[0] and o[1] <= s[1] for o in spans)]
    return [[x.strip() for x in body[a:b + 1] if x.strip() and not x.strip().startswith((";", "."))] for a, b in inner]


def instruction_counts():
    """VALU instructions per evaluation of the two hot loops, from the disassembly; {} where hipcc is absent."""
    from sph_code_amd import build as bld
    try:
        hipcc = bld.hipcc_path()
    except RuntimeError:
        return {}
    src = os.path.join(bld.CSRC, "sphx_rad.hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "sphx_rad.s")
        res = subprocess.run([hipcc] + bld.FLAGS + ["-S", "--cuda-device-only", "-o", out, src], capture_output=True, text=True)
        if res.returncode != 0:
            return {}
        asm = open(out).read()
    hdr = open(os.path.join(ROOT, "include", "sphx.h")).read()
    src_chunk = int(re.search(r"#define\s+SPHX_RAD_SRC_CHUNK\s+(\d+)", hdr).group(1))
    valu = lambda blk: sum(1 for x in blk if x.startswith("v_"))
    col = max(loops_of(asm, "_Z17rad_column_kernelILb0EE"), key=valu)          # the two-rays-per-lane loop
    pairs = sum(1 for x in col if x.startswith("v_cmp") and "_f64" in x)
    has = lambda blk, op: any(x.startswith(op) for x in blk)                    # the target loop: LDS reads and a square root
    dep = max((b for b in loops_of(asm, "_Z18rad_deposit_kernel") if has(b, "v_rsq_f64") and has(b, "ds_read")), key=valu)
    terms = src_chunk * sum(1 for x in dep if x.startswith("v_rsq_f64"))
    return dict(column_valu_per_pair=valu(col) / pairs, column_loop_valu=valu(col), column_loop_pairs=pairs,
                column_loop_lds_reads=sum(1 for x in col if x.startswith("ds_read")),
                deposit_valu_per_term=valu(dep) / terms, deposit_loop_valu=valu(dep), deposit_loop_terms=terms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--sources", type=int, default=32)
    ap.add_argument("--targets", type=int, default=125)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--mode", default="line")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from sph_code_amd import ics
    from sph_code_amd.sim import Simulation

    s = ics.polytrope_sphere(a.n, light=True, size_scale=ics.bench_size_scale(a.n))
    rs = np.random.RandomState(1)
    cross = 10.0 ** rs.uniform(-25.0, -21.0, a.n)
    lum = 10.0 ** rs.uniform(0.0, 4.0, a.sources)
    sim = Simulation(s, n_neigh=40)
    sim.step(1)
    st = sim.download()
    pick = rs.choice(a.n, a.sources + a.targets, replace=False)
    src, dst = st["points"][pick[:a.sources]].copy(), st["points"][pick[a.sources:]].copy()
    n_gas = int(np.count_nonzero(np.asarray(s["particle_type"]) != 1))
    sim.rad_transfer(src, lum, dst, cross, st["dt"], mode=a.mode)               # warm-up: buffers
    host, dev = [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        sim.rad_transfer(src, lum, dst, cross, st["dt"], mode=a.mode)
        host.append((time.perf_counter() - t0) * 1e3)
        dev.append(sim.rad_timing())
    med = {k: float(np.median([t[k] for t in dev])) for k in dev[0]}
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    issue = LANES_PER_CYCLE_PER_SIMD * 4 * cus * CLOCK_HZ                        # fp64 lane-instructions per second
    pairs = float(a.sources) * a.targets * a.n
    terms = float(a.sources) * a.targets * n_gas
    res = dict(tool="rad_rate", n=a.n, n_gas=n_gas, sources=a.sources, targets=a.targets, mode=a.mode, repeats=a.repeats,
               build=sim.ctx.build_info()["library"], compute_units=cus, clock_hz_assumed=CLOCK_HZ,
               ms_upload=med["upload"], ms_columns=med["columns"], ms_deposit=med["deposit"], ms_download=med["download"],
               ms_device=sum(med.values()), ms_host_call=float(np.median(host)),
               ray_particle_evaluations=pairs, ray_particle_per_s=pairs / (med["columns"] * 1e-3),
               src_dst_particle_evaluations=terms, src_dst_particle_per_s=terms / (med["deposit"] * 1e-3))
    ic = instruction_counts()
    res.update(ic)
    if ic:
        res["column_issue_bound_per_s"] = issue / ic["column_valu_per_pair"]
        res["column_share_of_issue_bound"] = res["ray_particle_per_s"] / res["column_issue_bound_per_s"]
        res["deposit_issue_bound_per_s"] = issue / ic["deposit_valu_per_term"]
        res["deposit_share_of_issue_bound"] = res["src_dst_particle_per_s"] / res["deposit_issue_bound_per_s"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
