"""GPU checks of supernova_impulse (nsc:1192-1204; include/sphx.h sphx_supernova_impulse) against the NumPy restatement
tests/sn_oracle.py: the selections and their sizes equal, d_vels, true_mass, vel and the accumulated velocities BIT FOR
BIT (a NaN equal to a NaN); against the reference's own results to the bound tests/test_sn_cpu.py derives.  The input
sets are tests/sn_fixture.py's; test_sn_cpu.py shows on the restatement what each is there for."""
import numpy as np
import pytest

import sn_fixture
import sn_oracle
from sn_fixture import same

pytestmark = pytest.mark.gpu


def gpu(c, **kw):
    import sph_code_amd.compat as nsc
    v, sels, info = nsc.supernova_impulses(*sn_fixture.args(c), full=True, **kw)
    return v, sels, info


def check(c, what, **kw):
    keep = [np.array(a, copy=True) for a in sn_fixture.args(c)]
    v, sels, info = gpu(c, **kw)
    for a, b in zip(keep, sn_fixture.args(c)):
        assert np.array_equal(a, b, equal_nan=True), what + ": an input was modified"
    v_ref, out = sn_oracle.supernova_impulses(*sn_fixture.args(c), **kw)
    assert len(sels) == len(out)
    for t, ((d_vels, ids), (d_ref, sel_ref, tm_ref, vel_ref)) in enumerate(zip(sels, out)):
        print(what, "star", t, "selected", ids.shape[0], "of", int(np.sum(c["ptypes"] == 0)), "true_mass", info["true_mass"][t])
        assert ids.dtype == np.int64 and np.array_equal(ids, sel_ref), (what, t)
        assert d_vels.shape == (ids.shape[0], 3) and same(d_vels, d_ref), (what, t)
        assert same(info["true_mass"][t], tm_ref) and same(info["vel"][t], vel_ref), (what, t)
    assert same(v, v_ref), what
    cnt = info["counts"]
    print(what, cnt)
    assert cnt["zero_distance"] == sn_oracle.counts(c["points"], c["masses"], c["ptypes"], c["stars"], **{
        k_: v_ for k_, v_ in kw.items() if k_ == "mass_displaced"})["zero_distance"]
    assert cnt["lds_sorts"] + cnt["global_sorts"] == len(out) + cnt["widenings"]
    return v, sels, info


@pytest.mark.parametrize("n,seed", [(257, 11), (2049, 12)])
def test_mixed_cloud_three_overlapping_stars(n, seed):
    c = sn_fixture.cloud(n, seed)
    _, _, info = check(c, "n=%d" % n)
    assert info["counts"]["lds_sorts"] >= 1 and info["counts"]["bad_mass"] == 0
    two = dict(c, stars=c["stars"][:2])
    check(two, "n=%d, two stars" % n)
    one = dict(c, stars=c["stars"][2:])
    check(one, "n=%d, the third star alone" % n)


def test_star_on_the_rim():
    check(sn_fixture.rim(2049, 13), "rim")


def test_first_row_heavier_than_the_limit_selects_nothing():
    v, sels, info = check(sn_fixture.heavy_first(257, 14), "heavy first")
    assert sels[0][1].shape[0] == 0 and info["vel"][0] == np.inf and info["true_mass"][0] == 0.0


def test_all_gas_selected_when_it_is_light():
    c = sn_fixture.light(257, 15)
    v, sels, info = check(c, "light")
    assert sels[0][1].shape[0] == int(np.sum(c["ptypes"] == 0)) and info["counts"]["lds_sorts"] >= 1


def test_tie_rule_on_the_mirrored_cloud():
    c = sn_fixture.mirrored()
    v, sels, info = check(c, "mirrored")
    ids = sels[0][1]
    assert ids.shape[0] == 99 and ids[-1] < c["mirror"][ids[-1]] and c["mirror"][ids[-1]] not in set(ids)


def test_nan_position_orders_last():
    c = sn_fixture.with_nan(sn_fixture.cloud(257, 16))
    v, sels, info = check(c, "nan")
    assert c["nan_row"] not in set(sels[0][1])
    c = sn_fixture.with_nan(sn_fixture.light(257, 17))
    v, sels, info = check(c, "nan, all selected")
    assert sels[0][1][-1] == c["nan_row"] and np.all(np.isnan(v[c["nan_row"]]))


def test_coincident_gas_row_gets_nan_and_is_counted():
    c = sn_fixture.coincident(257, 18)
    v, sels, info = check(c, "coincident")
    assert info["counts"]["zero_distance"] == 1 and np.all(np.isnan(v[c["zero_row"]]))
    assert np.all(np.isfinite(np.delete(v, c["zero_row"], axis=0)))


def test_widening_when_negative_masses_defeat_the_bound():
    c = sn_fixture.widening()
    v, sels, info = check(c, "widening")
    assert info["counts"]["widenings"] >= 1 and info["counts"]["bad_mass"] >= 10 and sels[0][1].shape[0] > 310


def test_global_sort_at_20011_light_rows():
    """12 B x 20011 candidates exceed the LDS of a CU: no workgroup can sort them there."""
    c = sn_fixture.light(20011, 19)
    c["ptypes"][c["ptypes"] == 2] = 0.0                       # every row but the star is gas
    c["masses"][c["ptypes"] == 0] = np.minimum(c["masses"][c["ptypes"] == 0], sn_fixture.M / 40000.0)
    v, sels, info = check(c, "n=20011")
    assert sels[0][1].shape[0] == 20010 and info["counts"]["global_sorts"] >= 1 and info["counts"]["candidates"] >= 20010


def test_partial_selection_beyond_the_lds_sort():
    """The refinement of the bound: 20010 gas rows of which about 9000 are selected - more than one LDS sort holds."""
    c = sn_fixture.cloud(20011, 20, n_stars=1, select=9000.0)
    v, sels, info = check(c, "n=20011, partial")
    n_sel = sels[0][1].shape[0]
    assert 4096 < n_sel < int(np.sum(c["ptypes"] == 0)) and info["counts"]["global_sorts"] >= 1
    assert info["counts"]["candidates"] < int(np.sum(c["ptypes"] == 0))     # the bound left rows out
    c = sn_fixture.cloud(20011, 21, n_stars=1, select=700.0)
    v, sels, info = check(c, "n=20011, small selection")
    assert info["counts"]["lds_sorts"] == 1 and info["counts"]["candidates"] <= 4096 and info["counts"]["widenings"] == 0


def test_other_limit_and_energy():
    c = sn_fixture.cloud(2049, 22)
    check(c, "other arguments", mass_displaced=0.37 * sn_fixture.M, supernova_energy=3.3e43)


@pytest.mark.parametrize("t", [0, 1])
def test_against_the_reference(t):
    import sph_code_amd.compat as nsc
    f = sn_fixture.golden()
    d_vels, ids = nsc.supernova_impulse(f["points"], f["mass"], int(f["stars"][t]), f["particle_type"])
    ref_d, ref_sel = f["d_vels_%d" % t], f["selected_%d" % t]
    assert np.array_equal(ids, ref_sel)
    bound = (ref_d.shape[0] + 4) * 2.0 ** -53 * np.abs(ref_d)
    print("star %d: worst |diff| / bound %.3g" % (t, np.max(np.abs(d_vels - ref_d) / bound)))
    assert np.all(np.abs(d_vels - ref_d) <= bound)
    with pytest.raises(ValueError):
        nsc.supernova_impulse(f["points"], f["mass"], f["stars"], f["particle_type"])


def test_same_bits_and_counts_on_every_call():
    for c in (sn_fixture.cloud(2049, 12), sn_fixture.widening(), sn_fixture.cloud(20011, 20, n_stars=1, select=9000.0)):
        a, b = gpu(c), gpu(c)
        assert same(a[0], b[0]) and a[2]["counts"] == b[2]["counts"]
        for (da, ia), (db, ib) in zip(a[1], b[1]):
            assert same(da, db) and np.array_equal(ia, ib)
        assert same(a[2]["true_mass"], b[2]["true_mass"]) and same(a[2]["vel"], b[2]["vel"])


def test_cap_too_small_is_refused_with_the_size_needed():
    import sph_code_amd.compat as nsc
    from sph_code_amd._lib import dp, ip
    c = sn_fixture.cloud(257, 11)
    _, out = sn_oracle.supernova_impulses(*sn_fixture.args(c))
    need = sum(o[1].shape[0] for o in out)
    ctx = nsc.context()
    pts, m, pt = (np.ascontiguousarray(c[k_], dtype=np.float64) for k_ in ("points", "masses", "ptypes"))
    v = np.array(c["velocities"])
    ku = np.array(c["stars"], dtype=np.int64)             # (a copy: changed below)
    cap = need - 1
    sel_count = np.full(3, -7, dtype=np.int64); sel_ids = np.full(cap, -7, dtype=np.int64); d_vels = np.full((cap, 3), -7.0)
    tm = np.full(3, -7.0); vel = np.full(3, -7.0); counts = np.full(6, -7, dtype=np.int64)

    def call(cap_):
        return ctx.lib.sphx_supernova_impulse(ctx.h, 257, dp(pts), dp(m), dp(pt), 3, ip(ku), sn_fixture.M,
                                              sn_oracle.SUPERNOVA_ENERGY * sn_oracle.KICK_FRACTION, dp(v), cap_, ip(sel_count),
                                              ip(sel_ids), dp(d_vels), dp(tm), dp(vel), ip(counts))
    assert call(cap) == -1
    msg = ctx.lib.sphx_last_error(ctx.h).decode()
    assert str(need) in msg and "cap" in msg, msg
    assert np.array_equal(v, c["velocities"]) and np.all(sel_count == -7) and np.all(sel_ids == -7) and np.all(d_vels == -7.0)
    assert np.all(tm == -7.0) and np.all(vel == -7.0) and np.all(counts == -7)
    sel_ids = np.full(need, -7, dtype=np.int64); d_vels = np.full((need, 3), -7.0)
    assert call(need) == 0                                       # ... and the exact size is enough
    assert np.array_equal(sel_count, [o[1].shape[0] for o in out]) and same(v, sn_oracle.supernova_impulses(*sn_fixture.args(c))[0])
    # a star outside [0, n), a limit that is not positive
    ku[1] = 257
    assert call(need) == -1
    ku[1] = c["stars"][1]
    with pytest.raises(ValueError):
        nsc.supernova_impulses(*sn_fixture.args(c), mass_displaced=0.0)
    # the drop-in's first guess of cap too small: it asks again with the size the error names
    first, nsc._SN_FIRST_CAP = nsc._SN_FIRST_CAP, 10
    try:
        check(c, "second call with the size needed")
    finally:
        nsc._SN_FIRST_CAP = first


# ---- the event on the resident state (include/sphx.h sphx_state_supernova_impulse), N unchanged --------------------
STATE_KEYS = ("points", "velocities", "total_accel", "E_internal", "T", "sizes", "densities", "num_densities", "visc_heat", "pressure")


def resident(K, steps, **kw):
    """A Simulation of phase_fixture's cloud at N = 2049, stepped -> (sim, the set, three of its stars, a limit that a
    fifth of the gas reaches)."""
    import phase_fixture as pf
    from sph_code_amd.sim import Simulation
    f = pf.state(2049, K, 15, 545)
    sim = Simulation(pf.sim_state(f), n_neigh=K, with_species=True, **kw)
    for _ in range(steps):
        sim.step(1, fixed_dt=f["fixed_dt"])
    pt = f["particle_type"]
    stars = np.nonzero(pt == 1)[0][:3].astype(np.int64)
    return sim, f, stars, 0.2 * float(np.sum(f["mass"][pt == 0]))


def snapshot(sim):
    st = sim.download()
    st.update(sim.download_composition())
    return st


def unchanged(a, b, but=()):
    return all(same(a[k_], b[k_]) for k_ in a if k_ not in but and k_ != "dt")


@pytest.mark.parametrize("K", [16, 40])
@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("energy,dt_0", [(1e44, None), (1e30, 1.0e3)], ids=["ct", "dt_0"])
def test_resident_event_equals_the_array_route(K, steps, energy, dt_0):
    import sph_code_amd.compat as nsc
    sim, f, stars, M = resident(K, steps)
    pt = f["particle_type"]
    before, nb = snapshot(sim), sim.neighbors()
    ev = sim.supernova_impulse(stars, dt_0=dt_0, mass_displaced=M, supernova_energy=energy)
    v_ref, sels, info = nsc.supernova_impulses(before["points"], before["mass"], stars, pt, before["velocities"], mass_displaced=M,
                                               supernova_energy=energy, full=True)
    ct_ref = nsc.crossing_time(nb, v_ref, before["sizes"], pt)
    after = snapshot(sim)
    assert same(after["velocities"], v_ref) and not same(v_ref, before["velocities"])
    assert unchanged(before, after, but=("velocities",)) and np.array_equal(sim.neighbors(), nb)
    for (d_a, i_a), (d_b, i_b) in zip(ev["selections"], sels):
        assert np.array_equal(i_a, i_b) and same(d_a, d_b) and 0 < i_a.shape[0] < int(np.sum(pt == 0))
    assert same(ev["true_mass"], info["true_mass"]) and same(ev["vel"], info["vel"]) and ev["counts"] == info["counts"]
    d0 = nsc.dt_0 if dt_0 is None else dt_0
    print("K=%d steps=%d: ct %.6g, dt_0/100 %.6g, selected %s" % (K, steps, ev["ct"], d0 / 100, ev["sel_count"]))
    assert same(ev["ct"], ct_ref) and same(ev["dt"], sn_oracle.event_dt(d0, ct_ref))
    assert (ev["dt"] == ev["ct"]) == (dt_0 is None)                       # each side of drv:358's min is met
    # the loop goes on: the step and the dust phase read the kicked state without a refusal
    sim.step(1, fixed_dt=ev["dt"])
    later = sim.download()
    assert np.all(np.isfinite(later["points"])) and not same(later["points"], before["points"])
    assert sim.supernova_impulse([])["dt"] is None and unchanged(snapshot(sim), dict(later, **sim.download_composition()))


def test_resident_event_refusals_leave_the_state_as_it_was(monkeypatch):
    import phase_fixture as pf
    import sph_code_amd.compat as nsc
    from sph_code_amd import _lib
    from sph_code_amd.sim import Simulation
    f = pf.state(2049, 16, 15, 545)
    stars = np.nonzero(f["particle_type"] == 1)[0][:2]
    M = 0.2 * float(np.sum(f["mass"][f["particle_type"] == 0]))

    def refused(sim, exc, words, ids=stars, **kw):
        before = snapshot(sim)
        with pytest.raises(exc, match=words) as e:
            sim.supernova_impulse(ids, mass_displaced=M, **kw)
        assert exc is ValueError or "error -4" in str(e.value)
        assert unchanged(before, snapshot(sim))

    sim = Simulation(pf.sim_state(f), n_neigh=16, with_species=True)
    refused(sim, RuntimeError, "before the first sphx_step")
    sim = Simulation(pf.sim_state(f), n_neigh=16, with_species=True, incremental=True)
    sim.step(1, fixed_dt=f["fixed_dt"])
    refused(sim, RuntimeError, "incremental")
    ctx = _lib.Context()
    try:
        sim = Simulation(pf.sim_state(f), n_neigh=16, with_species=True, ctx=ctx)
        sim.step(1, fixed_dt=f["fixed_dt"])
        refused(sim, ValueError, "outside", ids=[stars[0], 2049])
        refused(sim, ValueError, "outside", ids=[-1])
        st, nb = sim.download(), sim.neighbors()
        monkeypatch.setattr(nsc, "_ctx", ctx)                 # an array call on the Simulation's own context ...
        monkeypatch.setattr(nsc, "_nb_held", None)
        nsc.density(st["points"], f["mass"], f["particle_type"], nb, d=f["d"])    # ... uploads a list over the step's
        monkeypatch.undo()
        refused(sim, RuntimeError, "list is gone")
        sim.step(1, fixed_dt=f["fixed_dt"])
        assert sim.supernova_impulse(stars, mass_displaced=M)["dt"] > 0.0         # ... and after the next step it runs
    finally:
        ctx.close()
