#!/usr/bin/env python3
"""Golden vectors for the adaptive length scale and sizes from the reference DRIVER's own statements.

CONTAINER-ONLY TOOL (no-op when /root/reference is absent).  sph/code_running.py does not run as a whole
(make_golden_driver.py says why); its closing block

    code_running.py:493-540   vel_condition, the percentiles, d, the reverse counts, new_smoothing, sizes, densities_0

is straight-line code.  This tool reads the file at run time, takes the block BY LINE RANGE from the in-memory text (tabs
expanded, dedented from the `while` body) and `exec`s it in a namespace of seeded arrays carrying the names it reads.
What is stored is data only: the inputs put into the namespace and the values the block left behind.  No source text.

Two cases, each with gas, dust and stars and about a tenth of the rows fast:
    scale_a   densities_0 of the right length (drv:533)
    scale_b   a shorter densities_0 (drv:535: new_smoothing = 1.)
The lists hold every row itself and only entries inside [0, n): what the driver's np.unique needs to line up.
"""
import contextlib
import copy
import io
import os
import textwrap

import numpy as np

REF = "/root/reference/sph/code_running.py"
HERE = os.path.dirname(os.path.abspath(__file__))
FIRST, LAST = 493, 540
AU = 1.496e11
PARSEC = 3.0856775814913673e16


def block(first, last):
    lines = open(REF).read().split("\n")[first - 1:last]
    return compile(textwrap.dedent("\n".join(l.expandtabs(8) for l in lines)) + "\n",
                   "code_running.py:%d-%d" % (first, last), "exec")


class Stub(object):
    """Stands in for the modules the block assigns into or reads a constant from (nsc.d, constants.parsec)."""
    parsec = PARSEC
    d = None


def make_case(seed, n, K, short_d0):
    rng = np.random.RandomState(seed)
    points = rng.normal(size=(n, 3)) * 3.0 * PARSEC
    velocities = rng.normal(size=(n, 3)) * 2.0e4
    fast = rng.rand(n) < 0.1
    velocities[fast] *= 10.0                                     # well above 80 km/s
    particle_type = rng.choice([0., 1., 2.], size=n, p=[0.7, 0.1, 0.2])
    sizes = np.abs(rng.normal(size=n)) * 0.3 * PARSEC + 0.01 * PARSEC
    sizes[rng.rand(n) < 0.05] *= 40.0                            # rows the cap drv:537 catches
    densities = np.exp(rng.normal(size=n)) * 1e-20
    densities_0 = densities * np.exp(0.3 * rng.normal(size=n))
    densities[rng.rand(n) < 0.01] = 0.0                          # rho = 0: inf and NaN under the nan_to_num
    # the lists: every row itself, then a random number of other rows; a few rows alone and listed by nobody else
    alone = rng.rand(n) < 0.03
    others = np.flatnonzero(~alone)
    neighbor = np.full((n, K), n, dtype=np.int64)
    nontrivial_int = []
    for i in range(n):
        row = [i]
        if not alone[i]:
            cnt = rng.randint(0, K)
            pick = others[rng.randint(0, others.shape[0], size=cnt)]
            row += [int(p) for p in pick if p != i]
        row = np.array(row[:K], dtype=np.int64)
        neighbor[i, :row.shape[0]] = row
        nontrivial_int.append(row)
    num_nontrivial = np.array([r.shape[0] for r in nontrivial_int], dtype=np.int64)
    if short_d0:
        densities_0 = densities_0[:n - 7]
    return dict(points=points, velocities=velocities, particle_type=particle_type, sizes=sizes, densities=densities,
                densities_0=densities_0, neighbor=neighbor, num_nontrivial=num_nontrivial), nontrivial_int


def run_block(code, inp, nontrivial_int, N_INT_PER_PARTICLE, raise_factor):
    nsc = Stub()
    ns = dict(np=np, copy=copy, nsc=nsc, constants=Stub(), AU=AU, N_INT_PER_PARTICLE=N_INT_PER_PARTICLE, raise_factor=raise_factor,
              points=inp["points"].copy(), velocities=inp["velocities"].copy(), particle_type=inp["particle_type"].copy(),
              sizes=inp["sizes"].copy(), densities=inp["densities"].copy(), densities_0=inp["densities_0"].copy(),
              nontrivial_int=nontrivial_int, num_nontrivial=inp["num_nontrivial"].copy())
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
        exec(code, ns)
    n = inp["points"].shape[0]
    return dict(out_d=np.float64(ns["d"]), out_nsc_d=np.float64(nsc.d), out_max_dist=np.float64(ns["max_dist"]),
                out_n_slow=np.int64(np.count_nonzero(ns["vel_condition"] < 80000 ** 2)),
                out_exp_neighbor_count=np.asarray(ns["exp_neighbor_count"], dtype=np.int64),
                out_new_smoothing=np.broadcast_to(np.asarray(ns["new_smoothing"], dtype=np.float64), (n,)).copy(),
                out_sizes=ns["sizes"], out_densities_0=ns["densities_0"])


def main():
    if not os.path.exists(REF):
        print("reference not present: nothing to do")
        return
    code = block(FIRST, LAST)
    for name, seed, n, K, short in (("scale_a", 4931, 1500, 16, False), ("scale_b", 5401, 2048, 16, True)):
        inp, ragged = make_case(seed, n, K, short)
        N_INT, raise_factor = 40, 8.0
        out = run_block(code, inp, ragged, N_INT, raise_factor)
        np.savez_compressed(os.path.join(HERE, name + ".npz"), N_INT_PER_PARTICLE=np.int64(N_INT), raise_factor=np.float64(raise_factor),
                            **inp, **out)
        print(name, "n", n, "d", float(out["out_d"]), "n_slow", int(out["out_n_slow"]))


if __name__ == "__main__":
    main()
