"""GPU tests (-m gpu) of the dust phase on the resident state (Simulation.dust_phase, include/sphx.h
sphx_state_dust_phase) and the entry points that come with it.  The input sets, the one step each takes before the phase
and the conditions they meet are in tests/phase_fixture.py and tests/test_phase_cpu.py.  Every comparison is stage-wise on
identical inputs: the resident call against the array route bit for bit, the bookkeeping against tests/phase_oracle.py
within its derived bound, the step after a phase against the oracle's step from the downloaded state.

Run on an MI355X (DESIGN 5.13 says what has run and what has not)."""
import numpy as np
import pytest

import dust_oracle
import phase_fixture as pf
import phase_oracle as po
from step_oracle import oracle_step

pytestmark = pytest.mark.gpu

STAGES = ("density", "mass_chem", "f_un_chem", "frac_destruction", "frac_reuptake")
COMPOSITION = ("mass", "f_un", "mu_array", "gamma_array")
SPHERE = "sphere"


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def the_set(spec):
    return pf.sphere() if spec == SPHERE else pf.state(*spec)


def spec_id(spec):
    return spec if spec == SPHERE else pf.shape_id(spec)


def prepared(spec, forms="loop", with_drag=False, ctx=None, steps=1, **kw):
    """A Simulation of the set, stepped once under the set's fixed step -> (sim, the set)."""
    from sph_code_amd.sim import Simulation
    f = the_set(spec)
    K = f["neighbor"].shape[1]
    mode = dict(forms="loop", d=f["d"]) if forms == "loop" else {}
    sim = Simulation(pf.sim_state(f), n_neigh=K, with_species=True, with_drag=with_drag, ctx=ctx, **mode, **kw)
    for _ in range(steps):
        sim.step(1, fixed_dt=f["fixed_dt"])
    return sim, f


def array_route(nsc, sim, f, guard):
    """compat.dust_phase on what the Simulation holds -> (its result, the downloads)."""
    st, nb, comp = sim.download(), sim.neighbors(), sim.download_composition()
    out = nsc.dust_phase(st["points"], st["velocities"], nb, comp["mass"], comp["f_un"], comp["mu_array"], st["sizes"], st["T"],
                         f["particle_type"], d=f["d"], dt=f["dt"], guard=guard, full=True, **pf.tables(f))
    return out, st, nb, comp


@pytest.fixture(scope="module")
def nsc():
    import sph_code_amd.compat as nsc_mod
    nsc_mod.context()
    return nsc_mod


@pytest.mark.parametrize("forms", ["loop", "hydro_update"])
@pytest.mark.parametrize("spec", pf.SHAPES, ids=spec_id)
def test_neighbors_is_the_steps_exact_list(spec, forms):
    """1. After one step in either mode (hydro_update: the LDS passes, their slot lists and the forked streams have run
    over the list) Simulation.neighbors() holds, row by row as sets, the exact kNN of the uploaded points; column 0 is the
    particle itself; missing entries are N."""
    from oracle import sph_oracle as orc
    sim, f = prepared(spec, forms)
    n, K = len(f["mass"]), f["neighbor"].shape[1]
    nb = sim.neighbors()
    p, _ = orc.clamp_state(f["points"], f["velocities"])
    oi = orc.neighbors(p, np.inf, K, eps=0.0)[0]
    assert nb.shape == (n, K) and nb.dtype == np.int64
    assert np.array_equal(np.sort(nb, axis=1), np.sort(oi, axis=1))
    assert np.array_equal(nb[:, 0], np.arange(n))
    assert (nb == n).sum() == n * max(0, K - n) and nb.min() >= 0 and nb.max() <= n
    assert np.array_equal(sim.neighbors(), nb)


CASES = [(pf.SHAPES[0], "fraction", "loop"), (pf.SHAPES[1], "count", "hydro_update"), (pf.SHAPES[2], "fraction", "hydro_update"),
         (pf.SHAPES[3], "count", "loop"), (pf.SHAPES[4], "fraction", "loop"), (pf.SHAPES[5], "fraction", "hydro_update"),
         (pf.SHAPES[6], "count", "loop"), (SPHERE, "fraction", "hydro_update"), (SPHERE, "count", "loop")]


def assert_equals_array_route(nsc, sim, f, guard, what=""):
    """Simulation.dust_phase on the stepped `sim` against compat.dust_phase on its downloads -> (the resident result, the
    composition before).  The array route runs on compat's own context."""
    arr, st, nb, comp = array_route(nsc, sim, f, guard)
    res = sim.dust_phase(f["dt"], f["d"], guard=guard, full=True, **pf.tables(f))
    m, fu, mu, gam, totals, stages = arr
    print(what, guard, res["chem_counts"], res["dust_counts"], {k_: res[k_] for k_ in nsc.PHASE_TOTALS + nsc.PHASE_COUNTS},
          sim.phase_timing())
    for name in STAGES:
        assert same(res[name], stages[name]), name
    assert res["chem_counts"] == stages["chem_counts"] and res["dust_counts"] == stages["dust_counts"]
    for name in nsc.PHASE_TOTALS + nsc.PHASE_COUNTS:
        assert same(res[name], totals[name]), (name, res[name], totals[name])
    after = sim.download_composition()
    for name, a in zip(COMPOSITION, (m, fu, mu, gam)):
        assert same(after[name], a), name
    assert not same(after["mass"], comp["mass"]) or res["chem_counts"]["rows"] == 0
    st2 = sim.download()
    for key in st:
        assert same(st[key], st2[key]), key
    assert np.array_equal(sim.neighbors(), nb)
    assert np.all(np.isfinite(after["mass"])) and np.all(after["mass"] > 0)
    return res, comp


@pytest.mark.parametrize("spec,guard,forms", CASES, ids=["%s-%s-%s" % (spec_id(c[0]), c[1], c[2]) for c in CASES])
def test_resident_phase_equals_the_array_route(nsc, spec, guard, forms):
    """2. Simulation.dust_phase against compat.dust_phase on the downloaded state, neighbors() and download_composition():
    every stage output, the final composition, all counts and all totals with np.array_equal.  Nothing else of the state
    changes.  guard="count" is compared here and only here: bit for bit needs no margin."""
    sim, f = prepared(spec, forms)
    assert_equals_array_route(nsc, sim, f, guard, "%s %s" % (spec_id(spec), forms))


def test_phase_refreshes_the_drag_coefficients(nsc):
    """2, with drag on: after the phase mean_grain_mass and mean_cross are what Simulation forms from the new f_un."""
    sim, f = prepared(pf.SHAPES[1], "loop", with_drag=True)
    arr = array_route(nsc, sim, f, "fraction")[0]
    before = sim.download_drag()
    res = sim.dust_phase(f["dt"], f["d"], guard="fraction", full=True, **pf.tables(f))
    assert same(res["frac_reuptake"], arr[5]["frac_reuptake"]) and res["dust_counts"]["accepted"] > 0
    fu = sim.download_composition()["f_un"]
    assert same(fu, arr[1])
    mgm, mcs = sim.download_drag()
    assert np.array_equal(mgm, np.sum(nsc.grain_mass() * fu, axis=1)) and np.array_equal(mcs, np.sum(nsc.sigma_effective() * fu, axis=1))
    assert not np.array_equal(mgm, before[0])
    sim.step(1, fixed_dt=f["fixed_dt"])
    assert np.all(np.isfinite(sim.download()["velocities"]))


def test_bookkeeping_against_the_oracle(nsc):
    """3. compat.dust_bookkeeping on case (b)'s inputs (stub stages: NaNs in the fractions, NaN entries in f_un after chem,
    masses driven negative): every element within 1e-12 sum|terms| (phase_oracle's first-order bound), the mass resets
    and the NaN fills as exact index sets.  A filled entry comes back as 1e-15 / (its row's sum), about 1e-15; the
    sign that of the sum, which heavy losses make negative); the restatement's other entries are zero or above 1e-10 in
    magnitude (asserted), so the fills are the entries with 0 < |f| < 1e-14."""
    g = pf.load_golden("b")
    o = po.bookkeeping(g["mass_chem"], g["in_mu_array"], g["f_un_chem"], g["frac_destruction"], g["frac_reuptake"], g["mu_specie"],
                       g["gamma"], float(g["crit_mass"]), mass_before=g["in_mass"])
    assert o["reset_margin"] >= 1e6
    m, fu, mu, gam, totals = nsc.dust_bookkeeping(g["mass_chem"], g["in_mu_array"], g["f_un_chem"], g["frac_destruction"],
                                                  g["frac_reuptake"], mass_before=g["in_mass"], mu_specie=g["mu_specie"],
                                                  gamma=g["gamma"], crit_mass=float(g["crit_mass"]))
    for name, a in zip(po.BOOK_OUTPUTS, (m, fu, mu, gam)):
        print(name, "worst |x - ref| / bound: %.3g" % dust_oracle.worst_ratio(a, o[name], o[name + "_bound"]))
        dust_oracle.assert_within(name, a, o[name], o[name + "_bound"], "bookkeeping")
    assert np.array_equal(np.nonzero(m == float(g["crit_mass"]) / 200.)[0], o["reset"]) and totals["masses_reset"] == len(o["reset"])
    assert totals["nan_filled"] == len(o["filled"]) > 0
    is_fill = np.zeros(fu.shape, bool)
    is_fill[tuple(o["filled"].T)] = True
    assert not np.any((o["f_un"] != 0) & (np.abs(o["f_un"]) < 1e-10) & ~is_fill)    # the window below separates them
    assert np.array_equal(np.argwhere((fu != 0) & (np.abs(fu) < 1e-14)), o["filled"])
    for name in po.TOTALS:
        ref = o["totals"][name]
        assert (np.isnan(ref) and np.isnan(totals[name])) or abs(totals[name] - ref) <= o["totals_bound"][name], (name, totals[name], ref)


@pytest.mark.parametrize("forms", ["loop", "hydro_update"])
def test_next_step_reads_the_new_state(forms):
    """4. After the phase one more fused step, against the oracle's step from the downloaded state with the tolerances of
    tests/test_gpu_odd_shapes.py; in hydro_update mode download_species() meets the oracle's F formed from the new f_un.
    Control: the same oracle step fed the masses from before the phase fails the density comparison."""
    import oracle_bounds as ob
    from oracle import sph_oracle as orc
    sim, f = prepared(SPHERE, forms)
    n, K = len(f["mass"]), f["neighbor"].shape[1]
    before = sim.download_composition()
    res = sim.dust_phase(f["dt"], f["d"], guard="fraction", **pf.tables(f))
    comp, st = sim.download_composition(), sim.download()
    moved = int(np.count_nonzero(np.abs(comp["mass"] - before["mass"]) > 1e-6 * before["mass"]))
    print(forms, res["chem_counts"], res["dust_counts"], "masses moved:", moved)
    assert res["chem_counts"]["rows"] > 0 and res["chem_counts"]["rounds"] >= 3 and res["dust_counts"]["accepted"] > 0 and moved >= 1000
    s1 = dict(points=st["points"], velocities=st["velocities"], total_accel=st["total_accel"], E_internal=st["E_internal"], T=st["T"],
              particle_type=f["particle_type"], **comp)
    case = (forms, "cloud", n, K)
    sim.step(1, fixed_dt=f["fixed_dt"])
    got = sim.download()
    with np.errstate(all="ignore"):
        ref = oracle_step(case, s1, f["d"], False, f["fixed_dt"])
        old = oracle_step(case, dict(s1, mass=before["mass"]), f["d"], False, f["fixed_dt"])
    assert got["dt"] == pytest.approx(ref["dt"], rel=1e-12)
    R0 = np.max(np.abs(f["points"]))
    ex = np.max(np.abs(got["points"] - ref["points"])) / R0
    ev = np.max(np.abs(got["velocities"] - ref["velocities"])) / np.max(np.abs(ref["velocities"]))
    print("x err %.3g of the cloud size, v err %.3g of max|v|" % (ex, ev))
    assert ex <= 1e-12 and ev <= 1e-10
    np.testing.assert_allclose(got["sizes"], ref["sizes"], rtol=1e-9)
    np.testing.assert_allclose(got["densities"], ref["densities"], rtol=1e-9)
    assert not np.allclose(got["densities"], old["densities"], rtol=1e-9, atol=0)
    if forms == "hydro_update":
        p, v = orc.clamp_state(s1["points"], s1["velocities"])
        with np.errstate(all="ignore"):
            F = orc.hydro_update(ref["neighbor"], p, comp["mass"], ref["sizes"], comp["f_un"], f["particle_type"], s1["T"],
                                 comp["mu_array"], comp["gamma_array"], v)[5]
            F_old = orc.hydro_update(ref["neighbor"], p, comp["mass"], ref["sizes"], before["f_un"], f["particle_type"], s1["T"],
                                     comp["mu_array"], comp["gamma_array"], v)[5]
        Fg = sim.download_species()["f_un_neighbor"]
        ob.pos_close(Fg, F, "F from the new f_un")
        assert not np.allclose(Fg, F_old, rtol=1e-13, atol=0)


def test_refusals_leave_the_state_untouched(nsc):
    """5. Before the first step, without a composition, with s < 7, in incremental mode and with drag but no tables the
    call returns its error code and message, and download_composition() is unchanged."""
    from sph_code_amd import _lib
    from sph_code_amd._lib import dp
    from sph_code_amd.sim import Simulation
    f = pf.state(*pf.SHAPES[1])
    K, s0, t = f["neighbor"].shape[1], pf.sim_state(f), pf.tables(f)

    def refused(sim, code, words, **kw):
        before = sim.download_composition()
        with pytest.raises(RuntimeError if code != -1 else ValueError, match=words) as e:
            sim.dust_phase(f["dt"], f["d"], **dict(t, **kw))
        assert code == -1 or ("error %d" % code) in str(e.value)
        after = sim.download_composition()
        assert all(same(before[k_], after[k_]) for k_ in before)

    sim = Simulation(s0, n_neigh=K, with_species=True)
    refused(sim, -4, "before the first sphx_step")
    sim = Simulation(s0, n_neigh=K, with_species=False)
    sim.step(1, fixed_dt=f["fixed_dt"])
    refused(sim, -4, "no composition")
    few = dict(s0, f_un=np.ascontiguousarray(s0["f_un"][:, :6]))
    sim = Simulation(few, n_neigh=K, with_species=True)
    sim.step(1, fixed_dt=f["fixed_dt"])
    refused(sim, -4, "no composition", mu_specie=f["mu_specie"][:6], gamma=f["gamma"][:6], mineral_densities=f["mineral_densities"][:6],
            sputtering_yields=f["sputtering_yields"][:6])
    sim = Simulation(s0, n_neigh=K, with_species=True, incremental=True)
    sim.step(1, fixed_dt=f["fixed_dt"])
    refused(sim, -4, "incremental")
    with pytest.raises(RuntimeError, match="incremental"):
        sim.neighbors()
    # drag on, the two per-species tables missing: the C entry itself (Simulation always passes them)
    sim = Simulation(s0, n_neigh=K, with_species=True, with_drag=True, forms="loop", d=f["d"])
    sim.step(1, fixed_dt=f["fixed_dt"])
    before = sim.download_composition()
    pt = nsc.phase_tables(15, dt=f["dt"], **t)
    kv, kc, ks = pt["knots"]
    c = sim.ctx
    rc = c.lib.sphx_state_dust_phase(c.h, pt["dt"], f["d"], dp(pt["mu_specie"]), dp(pt["gamma"]), dp(pt["mineral_densities"]),
                                     dp(pt["sputtering_yields"]), dp(pt["mrn"]), nsc.k, nsc.amu, nsc.m_0, pt["crit_mass"],
                                     pt["critical_density"], pt["species_curve"].ctypes.data_as(_lib.c_int32_p), dp(kv), dp(kc), dp(ks),
                                     pt["guard"], None, None, None, None, None, None, None, None, None, None, None)
    assert rc == -1 and b"grain_mass" in c.lib.sphx_last_error(c.h)
    after = sim.download_composition()
    assert all(same(before[k_], after[k_]) for k_ in before)
    assert sim.dust_phase(f["dt"], f["d"], **t)["chem_counts"]["rows"] > 0          # ... and with them it runs


def test_list_guard_between_step_and_phase(nsc, monkeypatch):
    """5, the fifth refusal: array calls on the Simulation's own context between the step and the phase.  compat.neighbors
    there resets the context's processing order but leaves the step's list alone: neighbors() and the phase give the bits
    of a twin that was left in peace.  compat.density uploads a list of its own over the step's: neighbors() and the phase
    are refused, also after a later compat.neighbors (which clears the array calls' own flag), the state stays as it was,
    and after the next step both work again."""
    from sph_code_amd import _lib
    spec = pf.SHAPES[1]
    f = the_set(spec)
    ctxs = [_lib.Context(), _lib.Context()]
    try:
        sim, twin = (prepared(spec, "hydro_update", ctx=ctx)[0] for ctx in ctxs)
        nb = twin.neighbors()
        st = sim.download()
        monkeypatch.setattr(nsc, "_ctx", ctxs[0])            # compat's calls now run on the Simulation's context
        monkeypatch.setattr(nsc, "_nb_held", None)
        nsc.neighbors(st["points"], np.inf, nb.shape[1])
        assert np.array_equal(sim.neighbors(), nb)
        outs = [s.dust_phase(f["dt"], f["d"], guard="fraction", full=True, **pf.tables(f)) for s in (sim, twin)]
        for key in STAGES:
            assert same(outs[0][key], outs[1][key]), key
        comp = sim.download_composition()
        assert all(same(comp[k_], v) for k_, v in twin.download_composition().items())
        assert outs[0]["chem_counts"]["rows"] > 0
        nsc.density(st["points"], comp["mass"], f["particle_type"], nb, d=f["d"])
        for second_search in (False, True):
            if second_search:
                nsc.neighbors(st["points"], np.inf, nb.shape[1])
            with pytest.raises(RuntimeError, match="list is gone") as e:
                sim.dust_phase(f["dt"], f["d"], guard="fraction", **pf.tables(f))
            assert "error -4" in str(e.value)
            with pytest.raises(RuntimeError, match="list is gone"):
                sim.neighbors()
            assert all(same(comp[k_], v) for k_, v in sim.download_composition().items())
        monkeypatch.undo()
        for s in (sim, twin):
            s.step(1, fixed_dt=f["fixed_dt"])
        assert np.array_equal(sim.neighbors(), twin.neighbors())
        a, b = (s.dust_phase(f["dt"], f["d"], guard="fraction", full=True, **pf.tables(f)) for s in (sim, twin))
        assert all(same(a[k_], b[k_]) for k_ in STAGES)
    finally:
        for ctx in ctxs:
            ctx.close()


def test_repeatable_and_the_side_calls_see_the_new_state(nsc):
    """6. Two contexts prepared identically give identical bits after the phase.  rad_transfer after a phase gives the bits
    of compat.rad_transfer on the downloaded state with the new mass and mu_array.  sample() is held to arb_oracle's bound
    on that state, and misses it with the masses from before the phase: the samplers of the resident state and the
    compat.*_arb array forms sum the particles in different orders and never agreed in bits (tests/test_gpu_arb.py holds
    both to the same bound for that reason), so the bound is the sharpest statement there is.  (The array forms stand in for
    a fresh Simulation: one uploaded with the downloaded state would have to step before it has sizes, and would then sit
    at other positions.)"""
    import arb_oracle
    from sph_code_amd import _lib
    spec = pf.SHAPES[4]
    ctxs = [_lib.Context(), _lib.Context()]
    try:
        sims = [prepared(spec, "loop", ctx=ctx)[0] for ctx in ctxs]
        f = the_set(spec)
        outs = [s.dust_phase(f["dt"], f["d"], guard="fraction", full=True, **pf.tables(f)) for s in sims]
        comps = [s.download_composition() for s in sims]
        for key in outs[0]:
            assert outs[0][key] == outs[1][key] if not isinstance(outs[0][key], np.ndarray) else same(outs[0][key], outs[1][key]), key
        for key in COMPOSITION:
            assert same(comps[0][key], comps[1][key]), key
        sim, comp = sims[0], comps[0]
        st = sim.download()
        n = len(f["mass"])
        rs = np.random.RandomState(5)
        gas = np.nonzero(f["particle_type"] == 0)[0]
        src, dst = st["points"][gas[:3]].copy(), st["points"][gas[10:15]].copy()
        cross, lum = 10.0 ** rs.uniform(-25.0, -21.0, n), 10.0 ** rs.uniform(0.0, 4.0, 3)
        got = sim.rad_transfer(src, lum, dst, cross, 1e10, full=True)
        ref = nsc.rad_transfer(st["points"], f["particle_type"], comp["mass"], st["sizes"], cross, comp["mu_array"], src, lum, dst, 1e10,
                               full=True)
        old = nsc.rad_transfer(st["points"], f["particle_type"], f["mass"], st["sizes"], cross, f["mu_array"], src, lum, dst, 1e10,
                               full=True)
        assert all(same(a, b) for a, b in zip(got, ref)) and not all(same(a, b) for a, b in zip(got, old))
        lo, hi = st["points"].min(axis=0), st["points"].max(axis=0)
        q = np.ascontiguousarray(lo + rs.rand(65, 3) * (hi - lo))
        radius = float(np.max(st["sizes"]))
        samp = sim.sample(q, f["d"], fields=("density",), radius=radius)
        row_start, members = arb_oracle.brute_ball(st["points"], q, radius)
        o = arb_oracle.fields(points=st["points"], mass=comp["mass"], particle_type=f["particle_type"], sizes=st["sizes"], T=st["T"],
                              n_part=None, value=None, d=f["d"], m_0=nsc.m_0, arb_points=q, row_start=row_start, members=members)
        arb_oracle.assert_within("density", samp["density"], o["density"], o["density_bound"], what="sample after a phase")
        assert np.count_nonzero(samp["density"]) > 0
        o_old = arb_oracle.fields(points=st["points"], mass=f["mass"], particle_type=f["particle_type"], sizes=st["sizes"], T=st["T"],
                                  n_part=None, value=None, d=f["d"], m_0=nsc.m_0, arb_points=q, row_start=row_start, members=members)
        with pytest.raises(AssertionError):
            arb_oracle.assert_within("density", samp["density"], o_old["density"], o_old["density_bound"], what="control")
    finally:
        for ctx in ctxs:
            ctx.close()


def test_snapshot_carries_the_new_composition(tmp_path):
    """7. snapshot() after a phase, then from_snapshot(): the new mass, f_un, mu_array and gamma_array; a snapshot of a
    simulation that never ran a phase still takes them from the caller's state.  diagnostics() likewise."""
    from sph_code_amd.sim import Simulation
    sim, f = prepared(pf.SHAPES[1], "hydro_update")
    s0 = pf.sim_state(f)
    path0, path1 = str(tmp_path / "before.npz"), str(tmp_path / "after.npz")
    sim.snapshot(path0, s0)
    z0 = np.load(path0)
    assert all(same(z0[k_], s0[k_]) for k_ in COMPOSITION)
    sim.dust_phase(f["dt"], f["d"], guard="fraction", **pf.tables(f))
    comp = sim.download_composition()
    sim.snapshot(path1, s0)
    sim2, state2 = Simulation.from_snapshot(path1, with_species=True)
    assert all(same(state2[k_], comp[k_]) for k_ in COMPOSITION) and not same(state2["mass"], s0["mass"])
    again = sim2.download_composition()
    assert all(same(again[k_], comp[k_]) for k_ in COMPOSITION)
    # ... and diagnostics() weighs with the masses on the device, not the caller's stale ones
    dg, st = sim.diagnostics(s0), sim.download()
    assert np.array_equal(dg["momentum"], (st["velocities"] * comp["mass"][:, None]).sum(axis=0))
    assert not np.array_equal(dg["momentum"], (st["velocities"] * s0["mass"][:, None]).sum(axis=0))
