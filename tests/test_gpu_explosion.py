"""GPU tests (-m gpu) of the supernova explosion on the resident state: Simulation.supernova_explosion, include/sphx.h
sphx_state_download_rows / sphx_state_insert_rows (code_running.py:361-396, the block of the time loop that changes N).

The states are tests/phase_fixture.py's clouds and the golden sphere, with the masses of the exploding stars set so that
the number m of new rows falls into every regime of the buffers' head-room (sphx_ensure: bytes + bytes / 8 + 256): inside
it (nothing reallocated), beyond it for the composition rows alone, beyond it for every buffer, and across a multiple of
64 rows (npad).  The regime is worked out from that rule here and asserted against sphx_insert_last_info.

Every comparison is on identical inputs: the state after the event against compat.supernova_insert on the state
downloaded before it, bit for bit; the event's list and radii against compat.neighbors on the new positions; the step
after it against the array route on the downloaded post-event state (compat.neighbors, the sums, compat.leapfrog with
total_accel=None: dv = a dt, drv:482-485) - bit for bit in hydro_update mode, to the tolerances of SURVEY 8c for the loop
forms, as tests/test_gpu_parity.py compares them.

Run on an MI355X (DESIGN 5.17 says what has run and what has not)."""
import numpy as np
import pytest

import phase_fixture as pf

pytestmark = pytest.mark.gpu

SPHERE = "sphere"
STATE = ("points", "velocities", "E_internal", "T", "mass", "f_un", "mu_array", "gamma_array", "particle_type")


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@pytest.fixture(scope="module")
def nsc():
    import sph_code_amd.compat as nsc_mod
    nsc_mod.context()
    return nsc_mod


def the_set(spec, star_masses):
    """The set with the first len(star_masses) rows of type 1 weighing star_masses (solar) -> (set, star ids)."""
    import sph_code_amd.compat as nsc_mod
    f = dict(pf.sphere() if spec == SPHERE else pf.state(*spec))
    pt = f["particle_type"]                       # (a set with fewer stars than that: gas rows stand in)
    stars = np.concatenate((np.nonzero(pt == 1.0)[0], np.nonzero(pt == 0.0)[0]))[:len(star_masses)].astype(np.int64)
    m = np.array(f["mass"], dtype=np.float64)
    m[stars] = np.asarray(star_masses, dtype=np.float64) * nsc_mod.solar_mass
    f["mass"] = m
    return f, stars


def prepared(spec, star_masses, forms, steps, with_drag=False, **kw):
    from sph_code_amd.sim import Simulation
    f, stars = the_set(spec, star_masses)
    K = f["neighbor"].shape[1]
    mode = dict(forms="loop", d=f["d"]) if forms == "loop" else {}
    sim = Simulation(pf.sim_state(f), n_neigh=K, with_species=True, with_drag=with_drag, **mode, **kw)
    for _ in range(steps):
        sim.step(1, fixed_dt=f["fixed_dt"])
    return sim, f, stars, K


def snapshot(sim, drag=False):
    """Everything the Simulation holds, in the caller's order."""
    out = sim.download()
    out.update(sim.download_composition())
    out["particle_type"] = sim._ptype.copy()
    if drag:
        out["mean_grain_mass"], out["mean_cross"] = sim.download_drag()
    return out


def unchanged(a, b):
    return all(same(a[k_], b[k_]) for k_ in a if k_ != "dt")


def head_room(nbytes):
    nbytes = max(nbytes, 8)
    return nbytes + nbytes // 8 + 256


def expected_growth(n, m, sp, drag):
    """How many of the state's buffers an insertion of m rows behind n outgrows: 16 f64 arrays (18 with drag), the ids,
    the composition rows of sp doubles."""
    grown = (18 if drag else 16) * int((n + m) * 8 > head_room(n * 8))
    grown += int((n + m) * 4 > head_room(n * 4))
    grown += int((n + m) * sp * 8 > head_room(n * sp * 8))
    return grown


def hydro_array_step(nsc, cur, s, K, fixed_dt, old_accel):
    """One step in hydro_update mode through the array calls: compat.neighbors -> compat.hydro_update -> the leapfrog
    block.  compat.leapfrog takes the loop forms' terms (del_pressure / density, the viscous term as it is); fed with
    -hydro_accel over a density of 1 and nan_to_num(-visc_accel [gas]) it forms hydro_update mode's bits."""
    p, v = nsc.clamp_state(cur["points"], cur["velocities"])
    idx, _, _, _, h = nsc.neighbors(p, np.inf, K)
    pt = s["particle_type"]
    ha, va, vh, rho, nden, _, _ = nsc.hydro_update(idx, p, s["mass"], h, s["f_un"], pt, cur["T"], s["mu_array"], s["gamma_array"], v)
    g = (pt == 0.0).astype(np.float64)[:, None]
    with np.errstate(all="ignore"):
        vis = np.nan_to_num(-va * g)
    pn, vn, tot, E, T = nsc.leapfrog(p, v, old_accel, cur["E_internal"], s["mass"], s["mu_array"], s["gamma_array"], pt, -ha,
                                     np.ones(len(p)), (vis, vh), fixed_dt)
    return dict(points=pn, velocities=vn, total_accel=tot, E_internal=E, T=T, sizes=h, densities=rho, num_densities=nden, visc_heat=vh)


def assert_step(nsc, sim, f, K, forms, post, comp, old_accel, with_drag, what):
    """sim.step against the array route from `post` (+ the composition `comp`) with the previous acceleration old_accel
    (None: dv = a dt) -> (the download after the step, the array route's result)."""
    from test_gpu_parity import _close_to_array_path, _loop_array_step
    cur = dict(points=post["points"], velocities=post["velocities"], total_accel=old_accel, E_internal=post["E_internal"], T=post["T"])
    s = dict(mass=comp["mass"], particle_type=post["particle_type"], mu_array=comp["mu_array"], gamma_array=comp["gamma_array"],
             f_un=comp["f_un"])
    sim.step(1, fixed_dt=f["fixed_dt"])
    got = sim.download()
    if forms == "loop":
        ref, _ = _loop_array_step(nsc, cur, s, f["d"], K, False, with_drag, fixed_dt=f["fixed_dt"])
        _close_to_array_path(got, ref, post, what)
    else:
        ref = hydro_array_step(nsc, cur, s, K, f["fixed_dt"], old_accel)
        for key in ("sizes", "densities", "num_densities", "visc_heat", "total_accel", "points", "velocities", "E_internal", "T"):
            assert same(got[key], ref[key]), (key, what)
    return got, ref


# (spec, forms, steps before the event, star masses in solar masses, drag)
SMALL16, SMALL40, BIG40, BIG16 = (257, 16, 15, 513), (257, 40, 15, 544), (2049, 40, 15, 545), (2049, 16, 15, 517)
CASES = [
    (SMALL16, "loop", 1, (5.0,), False),             # m = 13: inside every head-room
    (SMALL16, "hydro_update", 1, (10.0,), False),    # m = 46: beyond the composition rows' head-room alone
    (SMALL40, "hydro_update", 3, (20.0, 12.0), False),   # m > 64: every buffer grows, N + m crosses 320
    (SMALL40, "loop", 3, (20.0,), True),             # ... with drag
    (BIG40, "loop", 1, (10.0, 8.0), False),          # inside at N = 2049
    (BIG16, "hydro_update", 3, (39.0,), False),      # m > 288: every buffer grows at N = 2049
    (SPHERE, "loop", 1, (10.0, 20.0), False),
    (SPHERE, "hydro_update", 3, (30.0,), False),
]


def case_id(c):
    return "%s-%s-steps%d-stars%d%s" % (c[0] if c[0] == SPHERE else pf.shape_id(c[0]), c[1], c[2], len(c[3]), "-drag" if c[4] else "")


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_event_and_the_steps_after_it(nsc, case):
    """1. and 2.: the state after the event, the event's list, and the two steps after it."""
    spec, forms, steps, star_masses, drag = case
    sim, f, stars, K = prepared(spec, star_masses, forms, steps, with_drag=drag)
    n = sim.n
    pre = snapshot(sim, drag)
    d_0 = float(np.median(pre["sizes"]))
    t_cmb = float(np.median(pre["T"])) if steps == 1 else nsc.t_cmb           # (the median: half of the old rows are clamped)
    # ---- the array route on the downloaded state, under the seed the resident call draws its noise under ----
    np.random.seed(4242)
    ex = nsc.supernova_explosion(pre["mass"], pre["points"], pre["velocities"], pre["E_internal"], stars, pre["f_un"], d_0=d_0)
    want = nsc.supernova_insert(pre, ex, t_cmb, mu_specie=f["mu_specie"], gamma=f["gamma"])
    np.random.seed(4242)
    res = sim.supernova_explosion(stars, d_0, t_cmb, mu_specie=f["mu_specie"], gamma=f["gamma"])
    m = res["n_dust"] + res["n_gas"]
    print(case_id(case), "n =", n, "m =", m, res["info"], res["dust_len"], sim.insert_timing())
    assert res["n_gas"] == len(stars) and res["n_dust"] == int(res["dust_len"].sum()) >= len(stars) and sim.n == n + m
    assert np.array_equal(res["new_ids"], np.arange(n, n + m))
    for a, b in zip(res["explosion"], ex):
        assert same(a, b)
    # the regime, from the head-room rule
    info = res["info"]
    assert info["reallocated"] == expected_growth(n, m, 16, drag) and info["appended"] == m and info["rewritten"] == len(stars)
    T_ext = np.concatenate((pre["T"], np.zeros(m)))
    assert info["clamped"] == int(np.count_nonzero(T_ext < t_cmb)) > 0
    # ---- 1. the state ----
    post = snapshot(sim, drag)
    for key in STATE + (("mean_grain_mass", "mean_cross") if drag else ()):
        assert same(post[key], want[key]), key
    assert np.all(post["particle_type"][n:n + res["n_dust"]] == 2.0) and np.all(post["particle_type"][n + res["n_dust"]:] == 0.0)
    assert same(post["total_accel"][:n], pre["total_accel"]) and not np.any(post["total_accel"][n:])
    for key in ("densities", "num_densities", "visc_heat", "pressure"):
        assert not np.any(post[key]), key
    p, _ = nsc.clamp_state(post["points"], post["velocities"])
    idx, _, _, _, h = nsc.neighbors(p, np.inf, K)
    nb = sim.neighbors()
    assert nb.shape == (n + m, K) and np.array_equal(np.sort(nb, axis=1), np.sort(idx, axis=1))
    assert np.array_equal(post["sizes"], h)
    # ---- 2. the step after it: dv = a dt on every row; the one after that averages again ----
    comp = {k_: post[k_] for k_ in ("mass", "f_un", "mu_array", "gamma_array")}
    got, ref = assert_step(nsc, sim, f, K, forms, post, comp, None, drag, "the step after the event")
    # ... and NOT dv = (a + a_old) / 2 dt on the old rows, which is what a state uploaded afresh with the old
    # accelerations (or zeros) integrates: the same array route with the previous acceleration padded to the new shape
    padded = np.concatenate((pre["total_accel"], np.zeros((m, 3))))
    cur = dict(points=post["points"], velocities=post["velocities"], total_accel=padded, E_internal=post["E_internal"], T=post["T"])
    s = dict(comp, particle_type=post["particle_type"])
    if forms == "loop":
        from test_gpu_parity import _loop_array_step
        avg = _loop_array_step(nsc, cur, s, f["d"], K, False, drag, fixed_dt=f["fixed_dt"])[0]
    else:
        avg = hydro_array_step(nsc, cur, s, K, f["fixed_dt"], padded)
    fin = np.all(np.isfinite(avg["velocities"][:n]) & np.isfinite(ref["velocities"][:n]) & np.isfinite(got["velocities"][:n]), axis=1)
    differ = np.any(avg["velocities"][:n] != ref["velocities"][:n], axis=1) & fin
    print("old rows on which the averaged update differs:", int(differ.sum()), "of", n)
    assert differ.sum() > 0
    if forms != "loop":
        assert np.all(np.any(got["velocities"][:n][differ] != avg["velocities"][:n][differ], axis=1))
    assert np.max(np.abs(got["velocities"][:n][fin] - ref["velocities"][:n][fin])) < \
        np.max(np.abs(got["velocities"][:n][fin] - avg["velocities"][:n][fin]))
    assert_step(nsc, sim, f, K, forms, dict(got, particle_type=post["particle_type"]), comp, got["total_accel"], drag,
                "the second step after the event")


def test_a_whole_pass_of_the_loop(nsc):
    """3. supernova_impulse, supernova_explosion, dust_phase, step on the resident state against the same chain of array
    calls (compat.dust_phase on the event's list)."""
    sim, f, stars, K = prepared(SMALL40, (12.0, 9.0), "loop", 1)
    n = sim.n
    pre = snapshot(sim)
    pt = pre["particle_type"]
    M = 0.2 * float(np.sum(pre["mass"][pt == 0.0]))
    d_0, t_cmb = float(np.median(pre["sizes"])), nsc.t_cmb
    # the array chain
    v1, _ = nsc.supernova_impulses(pre["points"], pre["mass"], stars, pt, pre["velocities"], mass_displaced=M)
    np.random.seed(77)
    ex = nsc.supernova_explosion(pre["mass"], pre["points"], v1, pre["E_internal"], stars, pre["f_un"], d_0=d_0)
    st = nsc.supernova_insert(dict(pre, velocities=v1), ex, t_cmb, mu_specie=f["mu_specie"], gamma=f["gamma"])
    p, _ = nsc.clamp_state(st["points"], st["velocities"])
    idx, _, _, _, h = nsc.neighbors(p, np.inf, K)
    m2, fu2, mu2, gam2, totals, _ = nsc.dust_phase(st["points"], st["velocities"], idx, st["mass"], st["f_un"], st["mu_array"], h, st["T"],
                                                  st["particle_type"], d=f["d"], dt=f["dt"], guard="fraction", full=True, **pf.tables(f))
    # the resident chain
    ev = sim.supernova_impulse(stars, mass_displaced=M)
    assert ev["sel_count"].sum() > 0 and same(sim.download()["velocities"], v1)
    np.random.seed(77)
    res = sim.supernova_explosion(stars, d_0, t_cmb, mu_specie=f["mu_specie"], gamma=f["gamma"])
    assert sim.n == n + res["n_dust"] + res["n_gas"]
    ph = sim.dust_phase(f["dt"], f["d"], guard="fraction", **pf.tables(f))
    for name in nsc.PHASE_TOTALS + nsc.PHASE_COUNTS:
        assert same(ph[name], totals[name]), name
    post = snapshot(sim)
    for key, a in (("mass", m2), ("f_un", fu2), ("mu_array", mu2), ("gamma_array", gam2), ("points", st["points"]),
                   ("velocities", st["velocities"]), ("T", st["T"]), ("E_internal", st["E_internal"]), ("sizes", h)):
        assert same(post[key], a), key
    assert not same(post["mass"], st["mass"])
    comp = dict(mass=m2, f_un=fu2, mu_array=mu2, gamma_array=gam2)
    assert_step(nsc, sim, f, K, "loop", post, comp, None, False, "the step of the pass")


def test_refusals_leave_the_state_untouched(nsc):
    """4. A call before any step; an incremental context; a duplicate id; an id >= N; S wrong."""
    from sph_code_amd import _lib
    from sph_code_amd._lib import dp
    from sph_code_amd.sim import Simulation
    f, stars = the_set(SMALL16, (5.0, 6.0))
    K = f["neighbor"].shape[1]
    d_0 = float(np.median(f["sizes"]))
    kw = dict(mu_specie=f["mu_specie"], gamma=f["gamma"])
    sim = Simulation(pf.sim_state(f), n_neigh=K, with_species=True)
    before = snapshot(sim)
    with pytest.raises(RuntimeError, match="-4"):
        sim.supernova_explosion(stars, d_0, nsc.t_cmb, **kw)
    assert unchanged(before, snapshot(sim)) and sim.n == len(f["mass"])
    inc = Simulation(pf.sim_state(f), n_neigh=K, with_species=True, incremental=True)
    inc.step(1, fixed_dt=f["fixed_dt"])
    before = snapshot(inc)
    with pytest.raises(RuntimeError, match="-4"):
        inc.supernova_explosion(stars, d_0, nsc.t_cmb, **kw)
    assert unchanged(before, snapshot(inc))
    sim.step(1, fixed_dt=f["fixed_dt"])
    before, nb = snapshot(sim), sim.neighbors()
    n = sim.n
    for bad in ([stars[0], stars[0]], [stars[0], n], [-1]):
        with pytest.raises(ValueError):
            sim.supernova_explosion(bad, d_0, nsc.t_cmb, **kw)
    # S wrong, a non-finite position: the C call itself
    c = sim.ctx
    one = np.ones(1)
    row14, row15 = np.ones((1, 14)), np.ones((1, 15))
    ids = np.array([stars[0]], dtype=np.int64)
    pos_nan = np.array([[0.0, np.nan, 0.0]])
    mus, gam = np.ascontiguousarray(f["mu_specie"]), np.ascontiguousarray(f["gamma"])
    for s, rowf, pos in ((14, row14, np.zeros((1, 3))), (15, row15, pos_nan)):
        rc = c.lib.sphx_state_insert_rows(c.h, s, 1, _lib.ip(ids), dp(one), dp(one), dp(rowf), 1, dp(pos), dp(np.zeros((1, 3))), dp(one),
                                          dp(np.zeros(1)), dp(one), dp(rowf), nsc.t_cmb, dp(mus), dp(gam), None, None, K, 0.0)
        assert rc == -1, (s, rc)
    assert unchanged(before, snapshot(sim)) and np.array_equal(sim.neighbors(), nb) and sim.n == n
    # ... and the state still steps as one that was never asked
    twin = Simulation(pf.sim_state(f), n_neigh=K, with_species=True)
    twin.step(1, fixed_dt=f["fixed_dt"])
    sim.step(1, fixed_dt=f["fixed_dt"])
    twin.step(1, fixed_dt=f["fixed_dt"])
    assert unchanged(snapshot(sim), snapshot(twin))


def test_two_events_and_the_side_calls_see_the_grown_state(nsc):
    """5. A second event inside the head-room the first created; then sample and rad_transfer on N + m rows."""
    sim, f, stars, K = prepared(SMALL40, (20.0, 5.0), "loop", 1)
    n = sim.n
    kw = dict(mu_specie=f["mu_specie"], gamma=f["gamma"])
    d_0 = float(np.median(f["sizes"]))
    np.random.seed(5)
    r1 = sim.supernova_explosion(stars[:1], d_0, nsc.t_cmb, **kw)
    m1 = r1["n_dust"] + 1
    assert r1["info"]["reallocated"] == expected_growth(n, m1, 16, False) == 18
    mid = snapshot(sim)
    np.random.seed(6)
    ex = nsc.supernova_explosion(mid["mass"], mid["points"], mid["velocities"], mid["E_internal"], stars[1:], mid["f_un"], d_0=d_0)
    want = nsc.supernova_insert(mid, ex, nsc.t_cmb, **kw)
    np.random.seed(6)
    r2 = sim.supernova_explosion(stars[1:], d_0, nsc.t_cmb, **kw)
    m2 = r2["n_dust"] + 1
    assert 0 < m2 <= (n + m1) // 8 and r2["info"]["reallocated"] == 0 and sim.n == n + m1 + m2
    assert np.array_equal(r2["new_ids"], np.arange(n + m1, n + m1 + m2))
    post = snapshot(sim)
    for key in STATE:
        assert same(post[key], want[key]), key
    N = sim.n
    # rad_transfer: the bits of the array call on the downloaded state
    rs = np.random.RandomState(3)
    cross = 10.0 ** rs.uniform(-25.0, -21.0, N)
    pt = post["particle_type"]
    src = post["points"][pt == 1.0][:3].copy()
    lum = 10.0 ** rs.uniform(0.0, 4.0, src.shape[0])
    dst = post["points"][N - 5:].copy()                       # (new rows among the targets)
    got = sim.rad_transfer(src, lum, dst, cross, f["fixed_dt"])
    ref = nsc.rad_transfer(post["points"], pt, post["mass"], post["sizes"], cross, post["mu_array"], src, lum, dst, f["fixed_dt"])
    for a, b in zip(got, ref):
        assert same(a, b)
    assert got[0].shape == (int(np.count_nonzero(pt != 1.0)),)
    # sample: the counts of the array call; the densities to the rounding of a positive sum in another order
    q = np.ascontiguousarray(post["points"][N - 8:] + 0.1 * d_0)
    smp = sim.sample(q, f["d"], fields=("density",), with_stats=True)
    narb = nsc.neighbors_arb(post["points"], q, post["sizes"])
    dens = nsc.density_arb(post["points"], q, post["mass"], pt, narb, d=f["d"])
    np.testing.assert_allclose(smp["density"], dens, rtol=1e-12, atol=0)
    assert np.count_nonzero(dens) > 0
    sim.step(1, fixed_dt=f["fixed_dt"])
    assert np.all(np.isfinite(sim.download()["points"]))


@pytest.mark.parametrize("gravity", [None, "direct", "tree"])
def test_a_state_without_its_composition_and_with_gravity(nsc, gravity):
    """with_species=False: the stars' composition rows come from the caller; mu_array and gamma_array of the other old rows
    stay as they are.  With self-gravity on, the step after the event runs on N + m rows."""
    from sph_code_amd.sim import Simulation
    f, stars = the_set(BIG16, (39.0, 30.0))
    K = f["neighbor"].shape[1]
    sim = Simulation(pf.sim_state(f), n_neigh=K, with_species=False, gravity=gravity)
    sim.step(1, fixed_dt=f["fixed_dt"])
    n = sim.n
    pre = snapshot(sim)
    assert "f_un" not in pre
    d_0, kw = float(np.median(pre["sizes"])), dict(mu_specie=f["mu_specie"], gamma=f["gamma"])
    np.random.seed(8)
    ex = nsc.supernova_explosion(pre["mass"], pre["points"], pre["velocities"], pre["E_internal"], stars, f["f_un"], d_0=d_0)
    want = nsc.supernova_insert(dict(pre, f_un=f["f_un"]), ex, nsc.t_cmb, **kw)
    with pytest.raises(ValueError, match="star_f_un"):
        sim.supernova_explosion(stars, d_0, nsc.t_cmb, **kw)
    np.random.seed(8)
    res = sim.supernova_explosion(stars, d_0, nsc.t_cmb, star_f_un=f["f_un"][stars], **kw)
    m = res["n_dust"] + res["n_gas"]
    assert res["info"]["reallocated"] == expected_growth(n, m, 0, False) == 17    # (no composition rows on the device)
    post = snapshot(sim)
    for key in ("points", "velocities", "E_internal", "T", "mass", "particle_type"):
        assert same(post[key], want[key]), key
    touched = np.concatenate((stars, np.arange(n, n + m)))
    old = np.setdiff1d(np.arange(n), stars)
    for key in ("mu_array", "gamma_array"):
        assert same(post[key][touched], want[key][touched]) and same(post[key][old], pre[key][old]), key
    sim.step(1, fixed_dt=f["fixed_dt"])
    got = sim.download()
    assert got["points"].shape == (n + m, 3) and np.all(np.isfinite(got["points"])) and np.all(np.isfinite(got["velocities"]))
    assert np.count_nonzero(got["densities"]) > 0.5 * n


def test_distributed_sim_refuses():
    from sph_code_amd.multigpu import DistributedSim
    with pytest.raises(NotImplementedError):
        DistributedSim.supernova_explosion(None, [0], 1.0, 2.7)
