"""GPU tests (-m gpu): the step's species / metallicity / AGB pass in every form against the CPU oracle, after every one of
three steps, on compositions that are not zero (tests/species_cases.py; tests/test_species_cpu.py checks, oracle only, that
no case is vacuous).

Per case the default context first (hydro_update and pairwise mode: the pass fused into pass 1's LDS kernel; loop mode: the
stand-alone LDS kernel).  The reference of a step is formed from the state the loop held before it - the IC, then the
previous download: clamp, SciPy's exact list, oracle.hydro_update's F on it.  F depends on the positions, h and the static
arrays only: nothing here compares trajectories.  Gates: F to oracle_bounds.RTOL_POS = 1e-13 (atol 0, every element),
metallicity rtol 1e-12 with the same NaN pattern, agb_dust rtol 1e-12 (atol 0) against
agb_oracle.calculate_interpolation at (m_i, the GPU's Z_i) on the live table.

Then the same case and steps in fresh contexts: SPHX_SPECIES_FUSED=0 (the stand-alone LDS kernel), SPHX_BLOB_SLOTS squeezed
(part of the references take the global-memory fallback inside the sweeps), both, and SPHX_SPECIES_LDS=0 (the gather form).
The species pass does not feed the dynamics: the downloaded states are bit-identical and the references are reused.  The LDS
forms agree bit for bit with each other (same expressions, same order); the gather form meets the oracle gates itself.

That a squeezed image overflows is argued from the lists, not read from a device counter: every list starts with the
particle itself (asserted on the oracle's list), so a full blob of 128 particles names at least 128 distinct particles
and an image of 100 slots must leave some of its references to the fallback wherever N >= 128.  That is SPHX_BLOB_SLOTS=100,
the K = 7 case's squeeze; 300 slots - the other cases' - hold less than half of the ~5 distinct particles per member a
blob names at K >= 16, but no count over the lists PROVES that for an unknown blob order, so those cases run a 100-slot
image as well.  N = 33 is one blob of 33: nothing can overflow there, every list has missing entries instead.
"""
import numpy as np
import pytest

import oracle_bounds as ob
import species_cases as sc

pytestmark = pytest.mark.gpu

STATE_KEYS = ("points", "velocities", "total_accel", "E_internal", "T", "sizes", "densities", "num_densities", "visc_heat",
              "pressure")


@pytest.fixture(scope="module")
def nsc():
    import sph_code_amd.compat as nsc_mod
    nsc_mod.context()
    return nsc_mod


def _run(case, s0, d, table, dt):
    """A fresh context (it reads the switches), three steps -> [(state, species outputs)] after every step."""
    from sph_code_amd.sim import Simulation
    forms, _, n, K, S, _ = case
    kw = dict(forms="loop", d=d, with_drag=(S == 15)) if forms == "loop" else \
        dict(visc_mode="pairwise" if forms == "pairwise" else "ref_axis0")
    sim = Simulation(s0, n_neigh=K, with_species=True, agb=table, **kw)
    out = []
    for _ in range(sc.NSTEPS):
        sim.step(1, fixed_dt=dt)
        out.append((sim.download(), sim.download_species()))
    return out


def _worst_rel(x, ref):
    with np.errstate(all="ignore"):
        err = np.abs(x - ref)
        return float(np.max(np.where(ref != 0, err / np.abs(ref), np.where(err == 0, 0., np.inf)))) if ref.size else 0.0


def _check_against_oracle(label, case, s0, got, F, table, spl):
    """One step's species outputs against the oracle's F (and what follows from it)."""
    from oracle import agb_oracle as ao
    n, S = case[2], case[4]
    assert ob.pos_close(got["f_un_neighbor"], F, label + " F") == n
    if table is None:
        assert "metallicity" not in got
        return
    Z = sc.metallicity_of(F, S)
    fin = np.isfinite(Z)
    gz = got["metallicity"]
    print("%-34s rows compared %8d  worst rel err %.3g (gate 1e-12)" % (label + " Z", fin.sum(), _worst_rel(gz[fin], Z[fin])))
    assert (np.isnan(gz) == ~fin).all(), "%s: NaN pattern of the metallicity differs on %d rows" % (
        label, (np.isnan(gz) != ~fin).sum())
    np.testing.assert_allclose(gz[fin], Z[fin], rtol=1e-12, atol=0)
    mapto, divisor = table[1], table[2]
    dust, _ = ao.calculate_interpolation(s0["mass"][fin], gz[fin], spl, sc.orc.MU_SPECIE[:S], np.ones((fin.sum(), S)),
                                         mapto=mapto, divisor=divisor)
    gd = got["agb_dust"][fin]
    print("%-34s rows compared %8d  worst rel err %.3g (gate 1e-12)" % (label + " agb_dust", fin.sum(), _worst_rel(gd, dust)))
    np.testing.assert_allclose(gd, dust, rtol=1e-12, atol=0)
    written = np.zeros(S, bool)
    written[np.asarray(mapto)] = True
    assert (gd[:, written] > 0).all() and (gd[:, ~written] == 0).all()
    # the yields differ between rows (not all: a third of the Z lie beyond the table's end knots and are clamped onto them, and
    # some knots carry the 1e-30 that stands for "no yield" - on the oracle two rows in three are distinct, 0.44 of a column)
    assert len(np.unique(gd, axis=0)) > fin.sum() // 2
    for q in np.flatnonzero(written):
        assert len(np.unique(gd[:, q])) > fin.sum() // 4, q


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_species_pass_vs_oracle_in_every_form(case, monkeypatch):
    forms, workload, n, K, S, with_agb = case
    cid = sc.case_id(case)
    s0, d = sc.live_state(case)
    dt = sc.fixed_dt(case, s0)
    table, spl = sc.case_table(case, s0)
    base = _run(case, s0, d, table, dt)
    refs, cur = [], s0
    for it, (st, sp) in enumerate(base):
        nb, h, F = sc.species_reference(s0, cur, K)
        assert (nb[:, 0] == np.arange(n)).all()                         # every list starts with the particle itself
        np.testing.assert_allclose(st["sizes"], h, rtol=2e-15, atol=0)
        _check_against_oracle("%s step %d" % (cid, it + 1), case, s0, sp, F, table, spl)
        refs.append(F)
        cur = st
    assert not np.array_equal(base[0][1]["f_un_neighbor"], base[2][1]["f_un_neighbor"])

    slots = sc.squeeze_slots(K)
    variants = [("separate", {"SPHX_SPECIES_FUSED": "0"}), ("squeezed", {"SPHX_BLOB_SLOTS": str(slots)}),
                ("separate+squeezed", {"SPHX_SPECIES_FUSED": "0", "SPHX_BLOB_SLOTS": str(slots)}),
                ("gather", {"SPHX_SPECIES_LDS": "0"})]
    if slots >= 128:
        variants.append(("separate+squeezed-100", {"SPHX_SPECIES_FUSED": "0", "SPHX_BLOB_SLOTS": "100"}))
        variants.append(("squeezed-100", {"SPHX_BLOB_SLOTS": "100"}))
    # a full blob of 128 particles names >= 128 distinct particles (its own members, asserted above): some squeeze of
    # the case holds fewer, so part of its references MUST overflow - but for the one blob of a case with N <= K
    squeezes = [int(env["SPHX_BLOB_SLOTS"]) for _, env in variants if "SPHX_BLOB_SLOTS" in env]
    assert min(squeezes) < 128 <= n or sc.all_in_every_list(case)
    for name, env in variants:
        for k_, v in env.items():
            monkeypatch.setenv(k_, v)
        res = _run(case, s0, d, table, dt)
        for k_ in env:
            monkeypatch.delenv(k_)
        for it, ((st, sp), (st0, sp0)) in enumerate(zip(res, base)):
            for key in STATE_KEYS:
                assert np.array_equal(st[key], st0[key], equal_nan=True), (name, it, key)
            assert st["dt"] == st0["dt"]
            assert set(sp) == set(sp0)
            if name == "gather":
                _check_against_oracle("%s step %d %s" % (cid, it + 1, name), case, s0, sp, refs[it], table, spl)
                # The other runs did go through the LDS forms: those add four partial sums over k mod 4, the gather form
                # adds in ascending k, so their F differ in bits somewhere.  (S > 16 has the gather form only.)  Were the
                # blob order missing, every run would be the gather form and "bit for bit" above would say nothing.
                assert np.array_equal(sp["f_un_neighbor"], sp0["f_un_neighbor"]) == (S > 16), (name, it)
            else:
                for key in sp0:
                    assert np.array_equal(sp[key], sp0[key], equal_nan=True), (name, it, key)


ARRAY_CASES = [(1000, 40, S) for S in sc.ARRAY_S] + [(n, K, 15) for n, K in sc.ARRAY_SHAPES[1:]]


@pytest.mark.parametrize("n,K,S", ARRAY_CASES, ids=["%d-%d-%d" % c for c in ARRAY_CASES])
def test_array_api_species_sums_on_live_compositions(nsc, n, K, S):
    """compat.hydro_update's F (pass_species_kernel) against the oracle on the GPU's own idx, h."""
    import sph_code_amd.ics as ics
    s = ics.two_phase(n)
    f = sc.live_composition(s, S, seed=7 * n + S)
    p, v = nsc.clamp_state(s["points"], s["velocities"])
    idx, _, _, nontriv, h = nsc.neighbors(p, np.inf, K)
    assert (nontriv == min(n, K)).all()
    args = (idx, p, s["mass"], h, f, s["particle_type"], s["T"], s["mu_array"], s["gamma_array"], v)
    F = nsc.hydro_update(*args)[5]
    with np.errstate(all="ignore"):
        Fref = sc.orc.hydro_update(*args)[5]
    assert F.shape == (S, n)
    assert ob.pos_close(F, Fref, "array API %d-%d-%d F" % (n, K, S)) == n
    has = sc.gas_in_support(s, s, idx, h)
    assert (Fref[:, has] > 0).all() and has.mean() >= 0.98


def test_array_api_refuses_33_species(nsc):
    import sph_code_amd.ics as ics
    s = ics.two_phase(1000)
    f = sc.live_composition(s, 33, seed=33)
    p, v = nsc.clamp_state(s["points"], s["velocities"])
    idx, _, _, _, h = nsc.neighbors(p, np.inf, 40)
    with pytest.raises(ValueError, match="species output needs f_un and 1 <= s <= 32"):   # SPHX_E_ARG
        nsc.hydro_update(idx, p, s["mass"], h, f, s["particle_type"], s["T"], s["mu_array"], s["gamma_array"], v)
