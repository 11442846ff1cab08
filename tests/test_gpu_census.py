"""GPU tests (-m gpu) of the census, the ordered selections and the stellar clock (include/sphx.h sphx_census and its
neighbours; drv:244, 339-342, 465-468, 604, 616-622, 636, 656-664).

Array calls: compat.census against the NumPy restatement tests/census_oracle.py BIT FOR BIT - the restatement forms the
per-row terms with the driver's expressions and sums them in the order of the library's ordered totals - at the chunk
edges N in {1, 2, 255, 256, 257, 513, 2049, 20011, 65793} (65793 = 257 * 256 + 1: the first N at which a lane of the second
stage adds two chunks), S in {1, 7, 8, 15, 16, 32} (both branches of the row sum, the padded widths) and the mixtures all
three types / no star / no dust / all dust.  Against the driver's own statements (tests/golden/census_a.npz, census_b.npz):
the exact items bit for bit, the sums within the derived bound 2 n_t 2^-53 sum|term| (tests/test_census_cpu.py).

Resident: every comparison is bit for bit between the resident call and the array call on the downloaded state, or between
twin Simulations."""
import os

import numpy as np
import pytest

import census_oracle as co
import phase_fixture as pf

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = (1, 2, 255, 256, 257, 513, 2049, 20011, 65793)
SPECIES = (1, 7, 8, 15, 16, 32)
MIXES = ("all", "no_star", "no_dust", "all_dust")
SUM_KEYS = ("gas_mass", "star_mass", "dust_mass", "nondust_mass", "total_mass", "momentum", "kinetic", "internal", "net_accel",
            "star_massfrac", "star_numfrac", "gas_mass_by_species", "star_mass_by_species", "dust_mass_by_species")
COUNT_KEYS = ("n_gas", "n_star", "n_dust", "n_nondust")
SMALL = pf.SHAPES[1]                     # n = 257, K = 40, S = 15
TWO_PHASE = pf.SHAPES[4]                 # n = 2049, K = 40, S = 32
ARGS = ("mass", "particle_type", "f_un", "mu_specie", "velocities", "total_accel", "E_internal")


@pytest.fixture(scope="module")
def nsc():
    import sph_code_amd.compat as nsc_mod
    nsc_mod.context()
    return nsc_mod


def same_bits(a, b):
    """Equal bit for bit, a NaN equal to a NaN."""
    if a is None or b is None:
        return a is None and b is None
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64))


def assert_census_equal(got, want, what, keys=SUM_KEYS):
    for key in COUNT_KEYS:
        assert got[key] == want[key], (what, key, got[key], want[key])
    assert same_bits(got["max_star_mass"], want["max_star_mass"]), (what, "max_star_mass")
    for key in keys:
        assert same_bits(got[key], want[key]), (what, key, got[key], want[key])


def args_of(s):
    return {k_: s[k_] for k_ in ARGS}


# ---------------------------------------------------------------------------------------------------------------------
# array calls
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_array_call_against_the_restatement(nsc, n):
    """Every S with all three types, every mixture at S = 15; also without a composition and without the dynamic arrays."""
    cases = [(S, "all") for S in SPECIES] + [(15, mix) for mix in MIXES[1:]]
    for S, mix in cases:
        s = co.make_state(1000 + n + S, n, S, mix)
        assert_census_equal(nsc.census(**args_of(s)), co.census(**args_of(s)), (n, S, mix))
    s = co.make_state(77 + n, n, 15)
    got = nsc.census(s["mass"], s["particle_type"])
    want = co.census(s["mass"], s["particle_type"])
    assert_census_equal(got, want, (n, "no composition"), ("gas_mass", "star_mass", "dust_mass", "nondust_mass", "total_mass"))
    assert got["gas_mass_by_species"] is None and got["kinetic"] is None and got["momentum"] is None


def test_masking_and_nan_cases(nsc):
    """A NaN mass, a NaN f_un row and a zero row sum in dust rows leave every gas and star quantity's bits alone and make the
    dust ones NaN exactly where the restatement has NaN; a zero row sum in a gas row poisons the gas sums alone."""
    s = co.make_state(31, 2049, 15)
    clean = nsc.census(**args_of(s))
    dust = np.flatnonzero(s["particle_type"] == 2)
    for kind in ("nan_mass", "nan_f_un", "zero_row", "all"):
        t = {k_: np.array(v) for k_, v in s.items()}
        if kind in ("nan_mass", "all"):
            t["mass"][dust[0]] = np.nan
        if kind in ("nan_f_un", "all"):
            t["f_un"][dust[1]] = np.nan
        if kind in ("zero_row", "all"):
            t["f_un"][dust[300]] = 0.0
        got, want = nsc.census(**args_of(t)), co.census(**args_of(t))
        for key in ("gas_mass", "star_mass", "nondust_mass", "star_massfrac", "gas_mass_by_species", "star_mass_by_species"):
            assert same_bits(got[key], clean[key]), (kind, key)
        assert_census_equal(got, want, kind)
        assert np.all(np.isnan(got["dust_mass_by_species"])), kind
        assert np.isnan(got["dust_mass"]) == (kind in ("nan_mass", "all"))
    t = {k_: np.array(v) for k_, v in s.items()}
    gas = np.flatnonzero(t["particle_type"] == 0)
    t["f_un"][gas[5]] = 0.0
    got = nsc.census(**args_of(t))
    assert_census_equal(got, co.census(**args_of(t)), "zero gas row")
    assert np.all(np.isnan(got["gas_mass_by_species"])) and same_bits(got["dust_mass_by_species"], clean["dust_mass_by_species"])
    assert same_bits(got["gas_mass"], clean["gas_mass"])


@pytest.mark.parametrize("name", ["census_a", "census_b"])
def test_the_driver_statements_fixtures(nsc, name):
    import test_census_cpu as cpu
    g = cpu.fixture(name)
    m, pt, f, ages, mus = g["mass"], g["particle_type"], g["f_un"], g["star_ages"], g["mu_specie"]
    assert np.array_equal(mus, nsc.mu_specie) and float(g["solar_mass"]) == nsc.solar_mass and float(g["year"]) == nsc.year
    # the schedule on the ages before the clock (drv:244, 339-341), the two near-1 stars of census_b among them
    sch = nsc.supernova_schedule(ages, pt, m)
    assert np.array_equal(sch["supernova_pos"], g["out_supernova_pos"])
    assert same_bits(sch["max_rel_age"], g["out_max_rel_age"])
    assert same_bits(sch["max_star_mass"], np.max(m[pt == 1] / nsc.solar_mass))
    # drv:604
    after = nsc.advance_star_ages(ages, pt, float(g["dt"]))
    assert same_bits(after, g["out_star_ages"]) and not same_bits(after, ages)
    # drv:616-622
    cen = nsc.census(m, pt, f, mus)
    print(name, {k_: cen[k_] for k_ in COUNT_KEYS}, nsc.census_last_timing())
    assert same_bits(cen["star_numfrac"], g["out_star_numfrac"])
    assert same_bits(nsc.select_rows(m, pt, 2, T=g["T"])["T"], g["out_dust_temps"]) and cen["n_dust"] == g["out_dust_temps"].shape[0]
    da, db = co.sum_bound(m[pt == 1], cen["n_star"]), co.sum_bound(m[pt != 2], cen["n_nondust"])
    b_ref, frac = float(np.sum(m[pt != 2])), float(g["out_star_massfrac"])
    print("star_massfrac", cen["star_massfrac"], frac)
    assert abs(cen["star_massfrac"] - frac) <= (da + abs(frac) * db) / (abs(b_ref) - db) + 2.0 ** -52 * abs(frac)
    # drv:656-664
    out = nsc.run_outputs(m, pt, f, after, float(g["OVERALL_AGE"]), mus)
    for key in ("AGB_condition", "AGB_list", "AGB_time_until", "AGB_metallicity", "AGB_composition"):
        assert out[key].shape == g["out_" + key].shape, key
        if key == "AGB_condition":
            assert np.array_equal(out[key], g["out_" + key])
        else:
            assert same_bits(out[key], g["out_" + key]), key
    for key, b in cpu.species_bounds(g).items():
        err = np.abs(out[key] - g["out_" + key])
        print(key, "worst |got - ref| / bound:", float(np.max(err / np.where(b > 0, b, 1.0))))
        assert np.all(err <= b), (key, err, b)


def test_selections_in_ascending_ids(nsc):
    s = co.make_state(8, 20011, 7)
    for ptype, window in ((0, None), (1, None), (2, None), (1, (1., 7.)), (0, (0.5, 2.0))):
        want = co.select(s["particle_type"], ptype, s["mass"], window)
        got = nsc.select_rows(s["mass"], s["particle_type"], ptype, T=s["T"], star_ages=s["star_ages"], f_un=s["f_un"], window=window)
        assert np.array_equal(got["ids"], want), (ptype, window)
        for key, src in (("mass", "mass"), ("T", "T"), ("star_ages", "star_ages"), ("f_un", "f_un")):
            assert same_bits(got[key], s[src][want]), (ptype, window, key)
    none = nsc.select_rows(s["mass"], np.zeros(20011), 1)
    assert none["ids"].shape == (0,)


def test_two_calls_in_a_row_and_any_row_order(nsc):
    s = co.make_state(4, 2049, 15)
    a, b = nsc.census(**args_of(s)), nsc.census(**args_of(s))
    assert_census_equal(a, b, "twice")
    for key in ("n_gas", "n_star", "n_dust"):
        assert a[key] > 0


def test_the_census_timer_is_apart_from_the_other_side_calls(nsc):
    import test_gpu_side_calls as side
    s = co.make_state(4, 2049, 15)

    def timings():
        t = side.timings(nsc)
        t["scale"] = nsc.scale_last_timing()
        t["census"] = nsc.census_last_timing()
        return t

    for fam in ("arb", "rad", "cool"):
        side.CALLS[fam](nsc)
    nsc.census(**args_of(s))
    for fam in ("census", "rad", "arb", "census", "cool"):
        before = timings()
        if fam == "census":
            nsc.census(**args_of(s))
        else:
            side.CALLS[fam](nsc)
        after = timings()
        assert tuple(after["census"]) == nsc.CENSUS_STAGES
        assert all(np.isfinite(v) and v >= 0.0 for v in after[fam].values()), after[fam]
        for other in after:
            if other != fam:
                assert after[other] == before[other], (fam, other)
    assert sum(nsc.census_last_timing().values()) > 0.0
    before = timings()
    nsc.select_rows(s["mass"], s["particle_type"], 2, T=s["T"])          # (a selection is not timed)
    nsc.advance_star_ages(s["star_ages"], s["particle_type"], 1.0)
    assert timings() == before


# ---------------------------------------------------------------------------------------------------------------------
# resident
# ---------------------------------------------------------------------------------------------------------------------
def ages_for(f, nsc):
    """Seeded star_ages for a set: the stars between 0 and 3e10 years, everything else -1, the first dust row -2."""
    pt = f["particle_type"]
    rs = np.random.RandomState(99)
    ages = np.where(pt == 1, rs.uniform(0., 3e10, size=pt.shape[0]) * nsc.year, -1.0)
    dust = np.flatnonzero(pt == 2)
    if dust.shape[0]:
        ages[dust[0]] = -2.0
    return ages


def prepared(spec, forms, nsc, steps=1, ages=True, **kw):
    from sph_code_amd.sim import Simulation
    f = pf.state(*spec)
    K = f["neighbor"].shape[1]
    mode = dict(forms="loop", d=f["d"]) if forms == "loop" else {}
    sim = Simulation(pf.sim_state(f), n_neigh=K, with_species=True, star_ages=ages_for(f, nsc) if ages else None, **mode, **kw)
    for _ in range(steps):
        sim.step(1, fixed_dt=f["fixed_dt"])
    return sim, f


def array_census(nsc, sim, mus):
    st, comp = sim.download(), sim.download_composition()
    return nsc.census(comp["mass"], sim._ptype, comp["f_un"], mus, st["velocities"], st["total_accel"], st["E_internal"]), st, comp


def assert_resident_equals_array(nsc, sim, f, what):
    mus = f["mu_specie"]
    want, st, comp = array_census(nsc, sim, mus)
    got = sim.census(mus)
    assert_census_equal(got, want, what)
    assert_census_equal(sim.census(mus), got, what + " twice")
    pt, ages = sim._ptype, sim.download_star_ages()
    assert same_bits(sim.dust_temperatures(), st["T"][pt == 2]), what
    assert sim.dust_temperatures().shape[0] == got["n_dust"]
    sch, want_s = sim.supernova_schedule(), nsc.supernova_schedule(ages, pt, comp["mass"])
    assert np.array_equal(sch["supernova_pos"], want_s["supernova_pos"]) and same_bits(sch["max_rel_age"], want_s["max_rel_age"])
    assert same_bits(sch["max_star_mass"], want_s["max_star_mass"])
    # the schedule in NumPy on the downloaded arrays, as the driver evaluates it
    pos, max_rel, max_m = co.schedule(ages, pt, comp["mass"])
    assert np.array_equal(sch["supernova_pos"], pos) and same_bits(sch["max_star_mass"], max_m)
    ro, want_r = sim.run_outputs(1.3e16, mus), nsc.run_outputs(comp["mass"], pt, comp["f_un"], ages, 1.3e16, mus)
    for key, v in want_r.items():
        assert same_bits(np.asarray(ro[key], dtype=np.float64), np.asarray(v, dtype=np.float64)), (what, key)
    whole = co.agb_outputs(comp["mass"], pt, comp["f_un"], ages, 1.3e16, mus)
    for key in ("AGB_list", "AGB_metallicity", "AGB_composition"):
        assert same_bits(ro[key], whole[key]), (what, key)
    return got


@pytest.mark.parametrize("spec,forms", [(SMALL, "hydro_update"), (TWO_PHASE, "loop")], ids=["n=257-hydro_update", "n=2049-loop"])
def test_resident_equals_the_array_call(nsc, spec, forms):
    """Before a step, after 1 and after 3 steps (the storage order has changed), after a dust_phase (mass and f_un have
    changed)."""
    sim, f = prepared(spec, forms, nsc, steps=0)
    first = assert_resident_equals_array(nsc, sim, f, "uploaded")
    sim.step(1, fixed_dt=f["fixed_dt"])
    one = assert_resident_equals_array(nsc, sim, f, "1 step")
    assert same_bits(one["total_mass"], first["total_mass"]) and same_bits(one["gas_mass_by_species"], first["gas_mass_by_species"])
    assert sim.last_dt() == sim.download()["dt"] == f["fixed_dt"]
    for _ in range(2):
        sim.step(1, fixed_dt=f["fixed_dt"])
    three = assert_resident_equals_array(nsc, sim, f, "3 steps")
    assert same_bits(three["total_mass"], first["total_mass"]) and not same_bits(three["kinetic"], first["kinetic"])
    sim.dust_phase(f["dt"], f["d"], guard="fraction", **pf.tables(f))
    after = assert_resident_equals_array(nsc, sim, f, "dust_phase")
    assert not same_bits(after["dust_mass_by_species"], three["dust_mass_by_species"])
    tm = sim.census_timing()
    assert tuple(tm) == nsc.CENSUS_STAGES and all(np.isfinite(v) and v >= 0.0 for v in tm.values()) and sum(tm.values()) > 0.0


def test_clock_advances_only_aging_stars(nsc):
    sim, f = prepared(SMALL, "hydro_update", nsc, steps=2)
    pt = f["particle_type"]
    ages = ages_for(f, nsc)
    star = np.flatnonzero(pt == 1)
    ages[star[0]] = -2.0                              # a star the clock leaves alone
    sim.set_star_ages(ages)
    dt = 3.3e12
    sim.advance_star_ages(dt)
    got = sim.download_star_ages()
    assert same_bits(got, co.advance(ages, pt, dt)) and same_bits(got, nsc.advance_star_ages(ages, pt, dt))
    moved = got != ages
    assert np.array_equal(np.flatnonzero(moved), star[1:]) and got[star[0]] == -2.0
    sim.step(1, fixed_dt=f["fixed_dt"])               # the storage order changes, the ages are by id
    sim.advance_star_ages(sim.last_dt())
    assert same_bits(sim.download_star_ages(), co.advance(got, pt, f["fixed_dt"]))


def test_behind_an_explosion_the_ages_grow_by_minus_two(nsc):
    import test_gpu_explosion as tex
    from sph_code_amd.sim import Simulation
    f, stars = tex.the_set(tex.SPHERE, (10.0,))
    ages = ages_for(f, nsc)
    sim = Simulation(pf.sim_state(f), n_neigh=f["neighbor"].shape[1], with_species=True, forms="loop", d=f["d"], star_ages=ages)
    twin = Simulation(pf.sim_state(f), n_neigh=f["neighbor"].shape[1], with_species=True, forms="loop", d=f["d"])
    for s_ in (sim, twin):
        for _ in range(2):
            s_.step(1, fixed_dt=f["fixed_dt"])
    n = sim.n
    d_0 = float(np.median(f["sizes"]))
    res = []
    for s_ in (sim, twin):
        np.random.seed(4242)
        res.append(s_.supernova_explosion(stars, d_0, nsc.t_cmb, mu_specie=f["mu_specie"], gamma=f["gamma"]))
    m_new = res[0]["n_dust"] + res[0]["n_gas"]
    assert m_new > 0 and sim.n == n + m_new
    got = sim.download_star_ages()
    assert got.shape == (n + m_new,) and same_bits(got[:n], ages) and np.all(got[n:] == -2.0)
    # the state itself is the twin's, which carries no ages: to the bit
    a, b = tex.snapshot(sim), tex.snapshot(twin)
    assert all(tex.same(a[k_], b[k_]) for k_ in a)
    assert res[0]["info"] == res[1]["info"]
    mus = f["mu_specie"]
    want, _, _ = array_census(nsc, sim, mus)
    assert_census_equal(sim.census(mus), want, "grown")
    sim.step(1, fixed_dt=f["fixed_dt"])
    sim.advance_star_ages(f["fixed_dt"])
    assert same_bits(sim.download_star_ages(), co.advance(got, sim._ptype, f["fixed_dt"]))
    want, _, _ = array_census(nsc, sim, mus)
    assert_census_equal(sim.census(mus), want, "grown, stepped")
    with pytest.raises(RuntimeError, match="no star_ages"):
        twin.download_star_ages()


def test_the_census_only_reads(nsc):
    """Twin Simulations, one calling census(), supernova_schedule() and dust_temperatures() between every pair of step,
    dust_phase, length_scale and download(): identical bits everywhere, download()["densities"] included."""
    import test_gpu_scale as tsc
    sims = [prepared(SMALL, "loop", nsc, steps=0)[0] for _ in range(2)]
    f = pf.state(*SMALL)

    def look(sim):
        sim.census(f["mu_specie"]); sim.supernova_schedule(); sim.dust_temperatures(); sim.run_outputs(0.0, f["mu_specie"])

    def both(call):
        out = []
        for q, sim in enumerate(sims):
            if q == 0:
                look(sim)
            out.append(call(sim))
            if q == 0:
                look(sim)
        return out

    def same_snapshots():
        a, b = both(tsc.snapshot)
        for key in a:
            assert tsc.same(a[key], b[key]), key

    both(lambda s_: s_.step(1, fixed_dt=f["fixed_dt"]))
    same_snapshots()
    a, b = both(lambda s_: s_.dust_phase(f["dt"], f["d"], guard="fraction", **pf.tables(f)))
    assert a == b
    same_snapshots()
    a, b = both(lambda s_: s_.length_scale(40, 8.0, full=True))
    assert all(tsc.same(a[k_], b[k_]) for k_ in a if k_ != "counts") and a["counts"] == b["counts"]
    both(lambda s_: s_.step(1, fixed_dt=f["fixed_dt"]))
    same_snapshots()
    a, b = both(lambda s_: s_.download())
    assert same_bits(a["densities"], b["densities"]) and np.any(a["densities"] != 0.0)


def test_refusals(nsc):
    import ctypes as C
    from sph_code_amd import _lib
    from sph_code_amd._lib import dp, ip
    from sph_code_amd.sim import Simulation
    f = pf.state(*SMALL)
    K = f["neighbor"].shape[1]
    # no state
    ctx = _lib.Context()
    tot, cnt, mx = np.zeros(13), np.zeros(4, dtype=np.int64), np.zeros(1)
    assert ctx.lib.sphx_state_census(ctx.h, None, dp(tot), ip(cnt), dp(mx)) == _lib.SPHX_E_STATE
    assert ctx.lib.sphx_state_set_star_ages(ctx.h, dp(np.zeros(4))) == _lib.SPHX_E_STATE
    assert ctx.lib.sphx_state_advance_star_ages(ctx.h, 1.0) == _lib.SPHX_E_STATE
    one = np.zeros(1, dtype=np.int64)
    assert ctx.lib.sphx_state_census_select(ctx.h, 2, 0, 1.0, 0.0, 0.0, 0, ip(one), None, None, None, None, None) == _lib.SPHX_E_STATE
    ctx.close()
    # without with_species: the rest is returned, the by-species entries are None; the C entry refuses the table
    plain = Simulation(pf.sim_state(f), n_neigh=K)
    cen = plain.census()
    want = nsc.census(f["mass"], f["particle_type"], None, None, f["velocities"], f["total_accel"], f["E_internal"])
    assert_census_equal(cen, want, "no species")
    assert cen["gas_mass_by_species"] is None and cen["dust_mass_by_species"] is None
    c = plain.ctx
    assert c.lib.sphx_state_census(c.h, dp(np.ones(15)), dp(np.zeros(58)), ip(cnt), dp(mx)) == _lib.SPHX_E_STATE
    with pytest.raises(RuntimeError, match="no composition"):
        plain.run_outputs(0.0)
    # the clock and the schedule before ages are set
    sim = Simulation(pf.sim_state(f), n_neigh=K, with_species=True)
    for call in (lambda: sim.advance_star_ages(1.0), sim.supernova_schedule, sim.download_star_ages, lambda: sim.run_outputs(0.0, f["mu_specie"])):
        with pytest.raises(RuntimeError, match="no star_ages"):
            call()
    assert sim.dust_temperatures().shape[0] == int(np.count_nonzero(f["particle_type"] == 2))       # (needs no ages)
    # a selection larger than the outputs is refused before anything is copied
    c = sim.ctx
    ids = np.full(4, -7, dtype=np.int64)
    rc = c.lib.sphx_state_census_select(c.h, 0, 0, 1.0, 0.0, 0.0, 4, ip(one), ip(ids), dp(np.zeros(4)), dp(np.zeros(4)), None, None)
    assert rc == -1 and one[0] == int(np.count_nonzero(f["particle_type"] == 0)) and np.all(ids == -7)
    from sph_code_amd.multigpu import DistributedSim
    with pytest.raises(NotImplementedError):
        DistributedSim.census(None)


def test_snapshot_carries_the_ages(nsc, tmp_path):
    from sph_code_amd.sim import Simulation
    sim, f = prepared(SMALL, "hydro_update", nsc, steps=1)
    sim.advance_star_ages(5.0e11)
    path = str(tmp_path / "snap.npz")
    sim.snapshot(path, pf.sim_state(f))
    back, _ = Simulation.from_snapshot(path, with_species=True)
    assert same_bits(back.download_star_ages(), sim.download_star_ages())
    plain, _ = prepared(SMALL, "hydro_update", nsc, steps=1, ages=False)
    plain.snapshot(path, pf.sim_state(f))
    assert "star_ages" not in np.load(path).files


def test_a_loop_without_an_n_sized_download(nsc, monkeypatch):
    """rad_phase, supernova_schedule, the event calls, dust_phase, step, length_scale, advance_star_ages(last_dt()) and
    census(), ending in run_outputs(), at n = 2049 with every N-sized download of the Simulation disabled."""
    import test_gpu_radphase as trp
    from sph_code_amd.sim import Simulation
    f = dict(trp.rad_set(TWO_PHASE))
    mus = f["mu_specie"]
    pt = f["particle_type"]
    stars = np.flatnonzero(pt == 1)
    m = np.array(f["mass"], dtype=np.float64)
    m[stars[:2]] = np.array([12.0, 9.0]) * nsc.solar_mass          # two progenitors the yield tables know
    m[stars[2:6]] = np.array([0.8, 2.0, 5.0, 7.5]) * nsc.solar_mass  # and stars on both sides of the AGB window
    f["mass"] = m
    ages = np.where(pt == 1, 0.0, -1.0)
    ages[stars[:2]] = 2.0 * nsc.luminosity_relation(m[stars[:2]] / nsc.solar_mass, lifetime=1) * 1e10 * nsc.year
    sim = Simulation(pf.sim_state(f), n_neigh=TWO_PHASE[1], with_species=True, forms="loop", d=f["d"], star_ages=ages)
    sim.step(1, fixed_dt=f["fixed_dt"])
    downloads = ("download", "download_composition", "neighbors", "download_star_ages", "download_sizes", "download_species")

    def refuse(*a, **kw):
        raise AssertionError("an N-sized download inside the loop")

    with monkeypatch.context() as mp:
        for name in downloads:
            mp.setattr(sim, name, refuse)
        age, exploded, rows = 0.0, 0, []
        for it in range(2):
            trp.resident(sim, f, full=False)
            sch = sim.supernova_schedule()
            if it == 0:
                assert np.array_equal(sch["supernova_pos"], stars[:2]) and abs(sch["max_rel_age"] - 2.0) < 1e-12
            if sch["supernova_pos"].shape[0] and it == 0:
                cen = sim.census(mus)
                ev = sim.supernova_impulse(sch["supernova_pos"], mass_displaced=0.2 * cen["gas_mass"])
                np.random.seed(77)
                ex = sim.supernova_explosion(sch["supernova_pos"], float(np.median(f["sizes"])), nsc.t_cmb, mu_specie=mus, gamma=f["gamma"])
                exploded = ex["n_dust"] + ex["n_gas"]
                dt = min(ev["dt"], f["fixed_dt"])             # (the sets' step: nothing moves far)
            else:
                dt = f["fixed_dt"]
            sim.dust_phase(f["dt"], f["d"], guard="fraction", **pf.tables(f))
            sim.step(1, fixed_dt=dt)
            sim.length_scale(40, 8.0)
            sim.advance_star_ages(sim.last_dt())
            age += sim.last_dt()
            cen = sim.census(mus)
            rows.append((cen["star_massfrac"], cen["star_numfrac"], sim.dust_temperatures().shape[0], cen["n_dust"]))
        out = sim.run_outputs(age, mus)
    assert exploded > 0 and sim.n == TWO_PHASE[0] + exploded
    assert all(r[2] == r[3] for r in rows) and all(np.isfinite(r[0]) and np.isfinite(r[1]) for r in rows)
    st, comp, got_ages = sim.download(), sim.download_composition(), sim.download_star_ages()
    assert np.all(got_ages[TWO_PHASE[0]:] == -2.0)
    want = nsc.run_outputs(comp["mass"], sim._ptype, comp["f_un"], got_ages, age, mus)
    for key, v in want.items():
        assert same_bits(np.asarray(out[key], dtype=np.float64), np.asarray(v, dtype=np.float64)), key
    assert out["AGB_list"].shape[0] >= 2
