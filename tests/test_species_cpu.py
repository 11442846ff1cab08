"""Oracle only (-m "not gpu"): no case of the species / metallicity / AGB sweep (tests/species_cases.py, run on the GPU
by tests/test_gpu_species.py) is vacuous, and the host-side argument checks of the AGB table."""
import numpy as np
import pytest

import species_cases as sc
from oracle import sph_oracle as orc


def test_live_composition_is_live():
    import sph_code_amd.ics as ics
    s = ics.two_phase(1000)
    for S in (1, 7, 15, 16, 20, 32):
        f = sc.live_composition(s, S, seed=S)
        assert f.shape == (1000, S) and (f > 0).all()
        assert np.array_equal(f, sc.live_composition(s, S, seed=S))
        if S > 6:
            mu = np.ones(S)
            mu[:min(S, 15)] = orc.MU_SPECIE[:min(S, 15)]
            z = sc.metal_fraction(f, mu)
            assert 3e-4 < z.min() < 6e-4 and 0.05 < z.max() < 0.1
            q = np.quantile(np.log10(z), [0.25, 0.5, 0.75])                      # log-uniform over 10^-3.5 ... 10^-1
            assert np.allclose(q, [-2.875, -2.25, -1.625], atol=0.12)


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_case_is_not_vacuous(case):
    """Three oracle steps in the case's mode and dt: the state stays finite and within ten cloud sizes; on the list of
    every step F is finite and > 0 in every species on every row with a gas neighbour inside its support and at most 2 %
    of the rows have no such neighbour (Z non-finite); with a table, the finite Z fall in at least four Z-intervals of
    the live table, some below its first and some above its last knot, and the masses in at least two mass intervals;
    between the lists of steps 1 and 3 at least 1 % of the rows changed their neighbour set (N <= K: every list names
    every particle at every step, so there it is the order of the list - by distance - that must have changed); every
    column of the composition takes more than N/2 distinct values across the gas rows."""
    forms, workload, n, K, S, with_agb = case
    s0, d = sc.live_state(case)
    gas = s0["particle_type"] == 0.
    for col in range(S):
        assert len(np.unique(s0["f_un"][gas, col])) > n / 2, col
    dt = sc.fixed_dt(case, s0)
    spl = sc.case_table(case, s0)[1]
    R0 = np.max(np.abs(s0["points"]))
    ref = dict(s0)
    lists = []
    for it in range(sc.NSTEPS):
        nb, h, F = sc.species_reference(s0, ref, K)
        lists.append(np.sort(nb, axis=1) if n > K else nb)
        has = sc.gas_in_support(s0, ref, nb, h)
        assert np.isfinite(F).all() and (F[:, has] > 0).all() and (F[:, ~has] == 0).all(), it
        assert (~has).mean() <= 0.02, (it, (~has).mean())
        if 6 < S <= 15:
            Z = sc.metallicity_of(F, S)
            assert np.array_equal(np.isfinite(Z), has)
            if with_agb:
                zi = sc.intervals(spl[0][0], Z[has])
                nz = len(spl[0][0]) - 3
                print("%s step %d: Z %.3g ... %.3g, Z-intervals %s" % (sc.case_id(case), it + 1, Z[has].min(), Z[has].max(),
                                                                      sorted(set(zi.tolist()))))
                assert len(set(zi.tolist())) >= 4 and (zi == -1).any() and (zi == nz).any(), (it, sorted(set(zi.tolist())))
                assert len(set(sc.intervals(spl[1][0], s0["mass"]).tolist())) >= 2
        ref = sc.oracle_step(case, ref, d, it == 0, dt)
        for key in ("points", "velocities", "sizes", "densities"):
            assert np.isfinite(ref[key]).all(), (it, key)
        assert np.max(np.abs(ref["points"])) < 10 * R0, (it, np.max(np.abs(ref["points"])) / R0)
    changed = (lists[0] != lists[2]).any(axis=1).mean()
    print("%s: rows whose neighbour set changed between steps 1 and 3: %.1f %%" % (sc.case_id(case), 100 * changed))
    assert changed >= 0.01


def test_agb_table_with_more_species_than_molecular_weights_is_refused():
    """Simulation(agb=...) and multigpu's set_agb hand mu_specie[:S] to a C call that reads S doubles: S > 15 must raise
    before anything is read (no kernel, no context)."""
    import sph_code_amd.compat as compat
    import sph_code_amd.ics as ics
    from sph_code_amd.multigpu import LibBackend
    from sph_code_amd.sim import Simulation
    s = ics.two_phase(64)
    table, _ = sc.live_table(sc.golden(), s["mass"])
    for S in (16, 20):
        s["f_un"] = sc.live_composition(s, S, seed=1)
        with pytest.raises(ValueError, match="mu_specie"):
            Simulation(s, n_neigh=8, with_species=True, agb=table)
        with pytest.raises(ValueError, match="mu_specie"):
            LibBackend.set_agb(None, S, table, compat.mu_specie, compat.solar_mass)
