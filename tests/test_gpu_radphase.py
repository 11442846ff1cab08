"""GPU tests of the radiative block of the time loop (code_running.py:247-316): the three elementwise array calls
(compat.rad_ionise, rad_heat_bookkeeping, rad_cool_bookkeeping; sphx_radphase.hip) against the fixtures the reference
driver's own statements left (tests/golden/make_golden_radphase.py) and against tests/radphase_oracle.py on seeded sets
at the sizes where the kernels change path, and the chain compat.rad_phase that joins them with rad_transfer and
rad_cooling.  Every element is compared, within the oracle's own per-element bound.  Then the block on the resident state
(Simulation.rad_phase, sphx_state_rad_phase): against the array route bit for bit, the step after it against the
oracle's step, a whole pass of the loop, the refusals and the side calls (the second half of this file)."""
import numpy as np
import pytest

import cool_fixture
import radphase_fixture as rf
import radphase_oracle as ro
import sph_code_amd.compat as nsc

pytestmark = pytest.mark.gpu

T_MAX = 1e4


def run_stage(case, stage):
    """The array call of a stage on a fixture's arguments -> dict by the oracle's names."""
    g = rf.load(case)
    c = rf.constants(g)
    mus, gam, cs = rf.tables(g)
    if stage == "ionise":
        a, (mu_s, cs_i, _) = rf.ionise_args(g)
        f, frac = nsc.rad_ionise(*a, mu_specie=mu_s, cross_sections=cs_i, full=True)
        return dict(f_un_new=f, frac_destroyed=frac)
    if stage == "heat":
        out = nsc.rad_heat_bookkeeping(*rf.heat_args(g), c["t_max"], t_cmb=c["t_cmb"], mu_specie=mus, gamma=gam, cross_sections=cs)
        return dict(zip(rf.HEAT_OUT + ("totals",), out))
    out = nsc.rad_cool_bookkeeping(*rf.cool_args(g), float(g["dt"]), c["t_max"], float(g["cooling_timescale"]), t_cmb=c["t_cmb"],
                                   mu_specie=mus, gamma=gam, cross_sections=cs)
    return dict(zip(rf.COOL_OUT + ("totals",), out))


def check_stage(got, o, what):
    for name in o:
        if name + "_bound" in o and not isinstance(o[name], dict):
            w = ro.assert_within(name, got[name], o[name], o[name + "_bound"], what)
            print("%s %-14s worst |difference| / bound = %.3g" % (what, name, w))
    if "totals" in o:
        for name in ro.TOTALS:
            want, have = o["totals"][name], got["totals"][name]
            assert (np.isnan(want) and np.isnan(have)) or abs(have - want) <= o["totals_bound"][name], (what, name, have, want)
        for name in ro.COUNTS:
            assert o["counts"][name][0] <= got["totals"][name] <= o["counts"][name][1], (what, name, got["totals"][name], o["counts"][name])


CASES = [("a", "ionise"), ("a", "heat"), ("a", "cool"), ("b", "heat"), ("b", "cool")]


@pytest.mark.parametrize("case,stage", CASES, ids=["%s-%s" % c for c in CASES])
def test_array_calls_meet_the_fixtures(case, stage):
    """Each array call on the reference's own inputs of its stage: every element within the oracle's bound of the oracle
    (which tests/test_radphase_cpu.py holds to the reference's results within the same bound), the clamp counts in the oracle's range,
    the totals within theirs; and the reference's results themselves within the same bound."""
    got, o, ref = run_stage(case, stage), rf.oracle(case, stage), rf.reference(case, stage)
    check_stage(got, o, "%s/%s" % (case, stage))
    for name, want in ref.items():
        ro.assert_within(name, got[name], want, o[name + "_bound"], "%s/%s against the reference" % (case, stage))


def seeded(n, S, seed):
    """Seeded inputs of the three calls that cross every regime: stars, dust, E_internal zero and negative, NaN and zero
    lf2, T on both sides of both limits, a composition entry of zero in a column the reactions read."""
    rs = np.random.RandomState(seed)
    pt = np.zeros(n)
    u = rs.rand(n)
    pt[u < 0.2] = 2.0
    pt[(u >= 0.2) & (u < 0.27)] = 1.0
    g = int(np.count_nonzero(pt != 1))
    f = rs.uniform(0.0, 1.0, (n, S)); f[:, :3] += 2.0
    f /= f.sum(axis=1)[:, None]
    f[::11, 0] = 0.0
    mus = np.concatenate([nsc.mu_specie, 1.0 + np.arange(32)])[:S].copy()
    gam = np.concatenate([nsc.gamma, np.full(32, 5. / 3)])[:S].copy()
    cs_i = np.concatenate([nsc.cross_sections, np.full(32, 1e-80)])[:S].copy()
    cs_d = np.concatenate([nsc.driver_cross_sections(), np.full(32, 3e-22)])[:S].copy()
    fd = np.concatenate([[0.96, 0.46, 0.74, 0, 0, 0.08], np.zeros(32)])[:S].copy()
    m = 1e30 * (1.0 + rs.rand(n))
    mu = np.sum(f * mus, axis=1) * rs.uniform(0.9, 1.1, n)
    E = m / (nsc.m_h * mu) * 1.6 * nsc.k * 10.0 ** rs.uniform(-1.0, 6.0, n)
    E[rs.rand(n) < 0.05] = 0.0
    E[rs.rand(n) < 0.05] *= -1.0
    lf2 = 10.0 ** rs.uniform(20, 40, g)
    lf2[rs.rand(g) < 0.03] = np.nan
    lf2[rs.rand(g) < 0.05] = 0.0
    energy = 10.0 ** rs.uniform(-30, -18, n) * np.where(rs.rand(n) < 0.15, -1.0, 1.0)
    energy[rs.rand(n) < 0.1] = 1e-8
    return dict(f=f, pt=pt, m=m, mu=mu, E=E, T=10.0 ** rs.uniform(-1.0, 6.0, n), lf2=lf2, mom=rs.normal(size=(g, 3)) * 10.0,
                vel=rs.normal(size=(n, 3)) * 1e3, sizes=1e14 * (1.0 + rs.rand(n)), energy=energy, mus=mus, gam=gam, cs_i=cs_i, cs_d=cs_d,
                fd=fd, ppj=2.3e17, dt=7.9e12)


def chain_on(s):
    """The three calls one after the other on a seeded set, each checked against the oracle on the same inputs."""
    f1, frac = nsc.rad_ionise(s["f"], s["pt"], s["m"], s["lf2"], s["fd"], s["ppj"], mu_specie=s["mus"], cross_sections=s["cs_i"], full=True)
    o = ro.ionise(s["f"], s["pt"], s["m"], s["lf2"], s["fd"], s["ppj"], s["mus"], s["cs_i"], nsc.amu)
    check_stage(dict(f_un_new=f1, frac_destroyed=frac), o, "ionise")
    heat = nsc.rad_heat_bookkeeping(f1, s["pt"], s["m"], s["mu"], s["E"], s["T"], s["lf2"], T_MAX, mu_specie=s["mus"], gamma=s["gam"],
                                    cross_sections=s["cs_d"])
    o = ro.heat_bookkeeping(f1, s["pt"], s["m"], s["mu"], s["E"], s["T"], s["lf2"], s["mus"], s["gam"], s["cs_d"], nsc.t_cmb, T_MAX, nsc.k,
                            nsc.m_h)
    check_stage(dict(zip(rf.HEAT_OUT + ("totals",), heat)), o, "heat")
    f2 = f1 * 1.07
    cool = nsc.rad_cool_bookkeeping(f2, s["energy"], s["pt"], s["m"], s["sizes"], heat[3], heat[4], s["vel"], s["lf2"], s["mom"], s["dt"],
                                    T_MAX, 2.0 * s["dt"], mu_specie=s["mus"], gamma=s["gam"], cross_sections=s["cs_d"])
    o = ro.cool_bookkeeping(f2, s["energy"], s["pt"], s["m"], s["sizes"], heat[3], heat[4], s["vel"], s["lf2"], s["mom"], s["mus"], s["gam"],
                            s["cs_d"], s["dt"], nsc.t_cmb, T_MAX, 2.0 * s["dt"], nsc.sb, nsc.k, nsc.m_h)
    check_stage(dict(zip(rf.COOL_OUT + ("totals",), cool)), o, "cool")
    return (f1, frac) + heat[:5] + cool[:6], (heat[5], cool[6])


@pytest.mark.parametrize("n,S", [(1, 15), (127, 6), (129, 15), (257, 6), (257, 16), (257, 32), (2049, 15), (2049, 32), (8193, 15)],
                         ids=lambda v: str(v))
def test_seeded_sets_across_the_tile_seams(n, S):
    """One tile and a lane (129), two and a lane (257), several chunks of the totals (2049, 8193), the smallest and the
    largest row (S = 6, 32), rows of even and odd length in LDS (16 / 15): every element of every output within the
    oracle's bound, the counts equal; and the same bits on a second call."""
    s = seeded(n, S, 100 * n + S)
    first, tot1 = chain_on(s)
    second = (nsc.rad_ionise(s["f"], s["pt"], s["m"], s["lf2"], s["fd"], s["ppj"], mu_specie=s["mus"], cross_sections=s["cs_i"], full=True) +
              nsc.rad_heat_bookkeeping(first[0], s["pt"], s["m"], s["mu"], s["E"], s["T"], s["lf2"], T_MAX, mu_specie=s["mus"], gamma=s["gam"],
                                       cross_sections=s["cs_d"]))
    for a, b in zip(first[:7], second[:7]):
        assert np.array_equal(a, b, equal_nan=True)
    assert all(second[7][k_] == tot1[0][k_] or (np.isnan(second[7][k_]) and np.isnan(tot1[0][k_])) for k_ in tot1[0])


def test_rows_are_normalised_for_every_particle_and_stars_keep_theirs():
    """nsc:1012 divides EVERY row by its sum - stars and dust included - while the reactions touch non-star rows alone."""
    s = seeded(300, 15, 5)
    s["f"] = s["f"] * 3.0
    f1 = nsc.rad_ionise(s["f"], s["pt"], s["m"], s["lf2"], s["fd"], s["ppj"])
    assert np.all(np.abs(np.sum(f1, axis=1) - 1.0) < 1e-14)
    star = s["pt"] == 1
    assert np.array_equal(f1[star], nsc.normalise_rows(s["f"])[star])
    assert not np.array_equal(f1[~star], nsc.normalise_rows(s["f"])[~star])


def test_nan_composition_rows_stay_where_they_are():
    s = seeded(300, 15, 6)
    s["f"][7, 3] = np.nan
    s["f"][8, 0] = np.nan
    first, _ = chain_on(s)
    assert np.isnan(first[0][7]).all() and np.isnan(first[0][8]).all()
    assert np.isfinite(np.delete(first[0], [7, 8], axis=0)).all()


def test_refusals():
    s = seeded(64, 15, 7)
    with pytest.raises(ValueError):
        nsc.rad_ionise(s["f"], s["pt"], s["m"], s["lf2"][:-1], s["fd"], s["ppj"])
    with pytest.raises(ValueError, match="6 <= s"):
        nsc.rad_ionise(s["f"][:, :5], s["pt"], s["m"], s["lf2"], s["fd"][:5], s["ppj"], mu_specie=s["mus"][:5], cross_sections=s["cs_i"][:5])
    with pytest.raises(ValueError, match="cooling_timescale"):
        nsc.rad_cool_bookkeeping(s["f"], s["energy"], s["pt"], s["m"], s["sizes"], s["E"], s["T"], s["vel"], s["lf2"], s["mom"], s["dt"], T_MAX,
                                 0.0)
    with pytest.raises(TypeError):
        nsc.rad_heat_bookkeeping(s["f"], s["pt"], s["m"], s["mu"], s["E"], s["T"], s["lf2"])      # t_max has no default


def cloud(n, K, seed, stars=0.02, dust=0.1, tree=False):
    """cool_fixture.cloud with sizes from the list (the distance to the last neighbour held), an E_internal, velocities,
    and the radiative setup by compat.rad_setup under a seeded generator."""
    c = cool_fixture.cloud(n, K, seed, dust=dust, stars=stars, tree=tree)
    dist = (cool_fixture._knn_tree if tree else cool_fixture._knn)(n, seed)[2]
    kk = min(K, n)
    c["sizes"] = np.maximum(dist[:, kk - 1], 1e13)
    c["masses"] = c["masses"] * 1e-3               # columns of optical depth about 0.1: the cloud is lit, and ionised
    c["d"] = c["d"] * 10.0                         # (h(m) of the cooling's kernel as it was)
    rs = np.random.RandomState(seed + 5)
    gam = np.sum(c["f_un"] * nsc.gamma, axis=1) / np.sum(c["f_un"], axis=1)
    c["E_internal"] = c["masses"] / (nsc.m_h * c["mu_array"]) * gam * nsc.k * c["T"] * 10.0 ** rs.uniform(-2.0, 0.5, n)
    c["velocities"] = rs.normal(size=(n, 3)) * 1e3
    stars_at = c["particle_type"] == 1
    c["masses"][stars_at] = nsc.solar_mass * 10.0 ** rs.uniform(-0.3, 1.6, int(stars_at.sum()))
    c["source_ids"], c["luminosities"], c["target_ids"] = nsc.rad_setup(c["particle_type"], c["masses"], [], c["dt"], rng=rs)
    if stars_at.any():
        c["frac_dest"], c["ppj"] = nsc.stellar_spectrum(c["masses"][stars_at])
    else:
        c["frac_dest"], c["ppj"] = np.zeros(15), 0.0
    return c


def phase_of(c, mode="line", full=True, dt=None):
    return nsc.rad_phase(c["positions"], c["velocities"], c["neighbor"], c["masses"], c["f_un"], c["mu_array"], c["sizes"], c["T"],
                         c["E_internal"], c["particle_type"], c["source_ids"], c["luminosities"], c["target_ids"], c["frac_dest"], c["ppj"],
                         c["dt"] if dt is None else dt, c["d"], T_MAX, 4.0 * c["dt"], mode=mode, full=full)


def check_chain(c, out, mode):
    """Every elementwise stage of the chain against the oracle on the chain's own previous outputs; the two physics
    stages against their own array calls."""
    f, mu, gam, E, T, vel, totals, st = out
    pt, m = c["particle_type"], c["masses"]
    lf2, mom, ext = nsc.rad_transfer(c["positions"], pt, m, c["sizes"], st["cross_array"], c["mu_array"], c["positions"][c["source_ids"]],
                                     c["luminosities"], c["positions"][c["target_ids"]], c["dt"], mode=mode)
    assert np.array_equal(lf2, st["lf2"], equal_nan=True) and np.array_equal(mom, st["momentum"], equal_nan=True)
    o = ro.ionise(c["f_un"], pt, m, st["lf2"], c["frac_dest"], c["ppj"], nsc.mu_specie, nsc.cross_sections, nsc.amu)
    check_stage(dict(f_un_new=st["f_un_ionised"], frac_destroyed=st["frac_destroyed"]), o, "chain ionise")
    cs = nsc.driver_cross_sections()
    o = ro.heat_bookkeeping(st["f_un_ionised"], pt, m, c["mu_array"], c["E_internal"], c["T"], st["lf2"], nsc.mu_specie, nsc.gamma, cs,
                            nsc.t_cmb, T_MAX, nsc.k, nsc.m_h)
    got = dict(mu_array=st["mu_heat"], gamma_array=st["gamma_heat"], cross_array=st["cross_heat"], E_internal=st["E_heat"], T=st["T_heat"])
    check_stage(got, {k_: v for k_, v in o.items() if k_ not in ("totals", "counts")}, "chain heat")
    for name in ("T_raised", "T_lowered"):
        assert o["counts"][name][0] <= totals["heat_" + name] <= o["counts"][name][1]
    final, energy, _ = nsc.rad_cooling(c["positions"], pt, m, c["sizes"], st["cross_heat"], st["f_un_ionised"], c["neighbor"], st["mu_heat"],
                                       st["T_heat"], c["dt"], d=c["d"])
    assert np.array_equal(final, f) and np.array_equal(energy, st["energy"])
    o = ro.cool_bookkeeping(f, st["energy"], pt, m, c["sizes"], st["E_heat"], st["T_heat"], c["velocities"], st["lf2"], st["momentum"],
                            nsc.mu_specie, nsc.gamma, cs, c["dt"], nsc.t_cmb, T_MAX, 4.0 * c["dt"], nsc.sb, nsc.k, nsc.m_h)
    got = dict(mu_array=mu, gamma_array=gam, cross_array=st["cross_array_out"], E_internal=E, T=T, velocities=vel)
    check_stage(got, {k_: v for k_, v in o.items() if k_ not in ("totals", "counts")}, "chain cool")
    assert abs(totals["E_before"] - float(np.sum(c["E_internal"]))) <= 1e-12 * float(np.sum(np.abs(c["E_internal"])))


@pytest.mark.parametrize("n,K,mode", [(257, 7, "line"), (257, 40, "segment"), (2049, 40, "line"), (2049, 7, "segment")],
                         ids=lambda v: str(v))
def test_chain_stage_by_stage(n, K, mode):
    """compat.rad_phase on seeded clouds that straddle the cooling's workgroup and the transfer's tile (256) and span
    several chunks at 2049: every stage checked, the heating does heat and the cooling does cool, and a second call
    gives the same bits."""
    c = cloud(n, K, 40 + n + K)
    assert len(c["source_ids"]) > 0 and len(c["target_ids"]) > 0
    out = phase_of(c, mode)
    check_chain(c, out, mode)
    assert not out[6]["skipped"] and np.any(out[7]["E_heat"] > c["E_internal"]) and np.any(out[7]["frac_destroyed"] > 0)
    again = phase_of(c, mode)
    for a, b in zip(out[:6], again[:6]):
        assert np.array_equal(a, b, equal_nan=True)
    assert again[6] == out[6]


def test_chain_beyond_one_scan_block_and_many_sources():
    """N = 8193 with K = 7 (beyond one scan block), and more stars selected than one source chunk of the transfer (16)."""
    c = cloud(8193, 7, 77, stars=0.01, tree=True)
    assert len(c["source_ids"]) > 16
    check_chain(c, phase_of(c), "line")


def test_chain_edges():
    """No star -> skipped, the inputs come back; zero targets is legal (lum_factor = 0: the light arrives unattenuated); N <= K with missing
    neighbours; all dust and one star: rad_transfer refuses, as the reference raises on the empty min."""
    c = cloud(300, 7, 3, stars=0.0)
    out = phase_of(c, full=False)
    assert out[6] == dict(skipped=True) and np.array_equal(out[0], c["f_un"]) and np.array_equal(out[3], c["E_internal"])
    assert np.array_equal(out[1], c["mu_array"]) and np.array_equal(out[4], c["T"]) and np.array_equal(out[5], c["velocities"])
    want = np.sum(c["f_un"] * nsc.gamma, axis=1) / np.sum(c["f_un"], axis=1)
    assert out[2].shape == want.shape and np.all(np.abs(out[2] - want) <= 1e-12 * want)        # gamma_array is no input
    c = cloud(300, 7, 4)
    lit = phase_of(c)[7]["lf2"]
    c["target_ids"] = np.zeros(0, np.int64)
    out = phase_of(c)
    assert np.all(out[7]["lf2"] >= lit) and np.any(out[7]["lf2"] > lit)      # lum_factor = 0: nothing is attenuated
    check_chain(c, out, "line")
    c = cloud(30, 40, 5, stars=0.1)
    assert np.any(c["neighbor"] == 30)
    check_chain(c, phase_of(c), "line")
    c = cloud(64, 7, 6, stars=0.0)
    c["particle_type"][:] = 2.0
    c["particle_type"][0] = 1.0
    c["source_ids"], c["luminosities"], c["target_ids"] = np.array([0]), np.array([1.0]), np.array([1, 2])
    with pytest.raises(ValueError):
        phase_of(c)


def test_side_calls_keep_their_bits_and_timers():
    """rad_transfer and rad_cooling between the new calls give their own first-call bits; the families' timers stay apart."""
    c = cloud(300, 7, 9)
    pt, m = c["particle_type"], c["masses"]
    cross = nsc.cross_array_of(c["f_un"])
    args = (c["positions"], pt, m, c["sizes"], cross, c["mu_array"], c["positions"][c["source_ids"]], c["luminosities"],
            c["positions"][c["target_ids"]], c["dt"])
    first = nsc.rad_transfer(*args)
    cool_first = nsc.rad_cooling(*cool_fixture.cloud_compat_args(c), d=c["d"])
    phase_of(c)
    rad_t, cool_t = nsc.rad_last_timing(), nsc.cool_last_timing()
    s = seeded(300, 15, 10)
    nsc.rad_ionise(s["f"], s["pt"], s["m"], s["lf2"], s["fd"], s["ppj"])
    own = nsc.radphase_last_timing()
    assert own["kernel"] > 0
    assert nsc.rad_last_timing() == rad_t and nsc.cool_last_timing() == cool_t
    for a, b in zip(first, nsc.rad_transfer(*args)):
        assert np.array_equal(a, b, equal_nan=True)
    for a, b in zip(cool_first, nsc.rad_cooling(*cool_fixture.cloud_compat_args(c), d=c["d"])):
        assert np.array_equal(a, b)
    assert nsc.radphase_last_timing() == own


# =====================================================================================================================
# the block on the resident state: Simulation.rad_phase (include/sphx.h sphx_state_rad_phase)
# =====================================================================================================================
import functools  # noqa: E402

import phase_fixture as pf  # noqa: E402
from step_oracle import oracle_step  # noqa: E402

PHASE_DT = 7.884e9                                # dt_0 / 1000: the cloud is heated and ionised, not saturated
FINALS = ("f_un", "mu_array", "gamma_array", "E_internal", "T", "velocities")


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@functools.lru_cache(maxsize=None)
def rad_set(spec, bright=False):
    """pf.state(*spec) (gas with ionised shares, dust, 2 % stars) with what the radiative block needs beside it: every
    star a source with a seeded luminosity of 10^U(0, 3) solar ones (the cloud's particles weigh 3e22 kg, so the
    reference's mass-luminosity law would leave it dark), targets by the reference's rule under a seeded generator, the
    spectrum of a nominal set of stars, tables of S entries.  bright: the luminosities 1e32 times those - the radiation's
    impulse (nsc:965 leaves it in units of a solar luminosity too small: 1e-29 m/s here) then moves the velocities by a
    visible amount, while the heating ends at the t_max clamp."""
    f = dict(pf.state(*spec))
    n, K, S, seed = spec
    rs = np.random.RandomState(seed + 77)
    pt = f["particle_type"]
    src = np.nonzero(pt == 1)[0].astype(np.int64)
    others = np.nonzero(pt != 1)[0]
    dst = others[rs.rand(len(others)) < len(others) ** -0.65].astype(np.int64)
    fd15, ppj = nsc.stellar_spectrum(nsc.solar_mass * np.array([1.0, 3.0, 8.0, 20.0]))
    pad = lambda a, fill: np.concatenate([np.asarray(a, dtype=np.float64), np.full(32, fill)])[:S].copy()
    f.update(source_ids=src, luminosities=10.0 ** rs.uniform(0.0, 3.0, len(src)) * (1e32 if bright else 1.0), target_ids=dst, frac_dest=pad(fd15, 0.0), ppj=ppj,
             tables=dict(mu_specie=f["mu_specie"], gamma=f["gamma"], cross_sections=pad(nsc.cross_sections, 1e-80),
                         driver_cross=pad(nsc.driver_cross_sections(), 3e-22)))
    return f


def rad_prepared(spec, forms="loop", with_drag=False, ctx=None, bright=False, **kw):
    from sph_code_amd.sim import Simulation
    f = rad_set(spec, bright)
    K = f["neighbor"].shape[1]
    mode = dict(forms="loop", d=f["d"]) if forms == "loop" else {}
    sim = Simulation(pf.sim_state(f), n_neigh=K, with_species=True, with_drag=with_drag, ctx=ctx, **mode, **kw)
    sim.step(1, fixed_dt=f["fixed_dt"])
    return sim, f


def rad_args(f):
    return (f["source_ids"], f["luminosities"], f["target_ids"], f["frac_dest"], f["ppj"])


def rad_array_route(sim, f, mode="line", full=True):
    """compat.rad_phase on what the Simulation holds -> (its result, the downloads)."""
    st, nb, comp = sim.download(), sim.neighbors(), sim.download_composition()
    out = nsc.rad_phase(st["points"], st["velocities"], nb, comp["mass"], comp["f_un"], comp["mu_array"], st["sizes"], st["T"],
                        st["E_internal"], f["particle_type"], *rad_args(f), PHASE_DT, f["d"], T_MAX, 4.0 * PHASE_DT, mode=mode, full=full,
                        **f["tables"])
    return out, st, nb, comp


def resident(sim, f, mode="line", full=True):
    return sim.rad_phase(PHASE_DT, f["d"], *rad_args(f), T_MAX, 4.0 * PHASE_DT, mode=mode, full=full, **f["tables"])


def finals_of(sim):
    st, comp = sim.download(), sim.download_composition()
    return dict(f_un=comp.get("f_un", np.zeros(0)), mu_array=comp["mu_array"], gamma_array=comp["gamma_array"], E_internal=st["E_internal"], T=st["T"],
                velocities=st["velocities"]), st, comp


def assert_equals_array_route(sim, f, mode):
    arr, st, nb, comp = rad_array_route(sim, f, mode)
    res = resident(sim, f, mode)
    totals, stages = arr[6], arr[7]
    for name in sim.RADPHASE_STAGES:
        assert same(res[name], stages[name]), name
    for name, want in totals.items():
        assert same(res[name], want), (name, res[name], want)
    after, st2, comp2 = finals_of(sim)
    for name, want in zip(FINALS, arr[:6]):
        assert same(after[name], want), name
    for key in ("points", "total_accel", "sizes", "densities", "num_densities", "visc_heat", "pressure", "dt"):
        assert same(st[key], st2[key]), key                          # (pressure: the previous temperature stays the last step's)
    assert same(comp["mass"], comp2["mass"]) and np.array_equal(sim.neighbors(), nb)
    return res, st, after


R_CASES = [(pf.SHAPES[0], "loop", "line", False), (pf.SHAPES[1], "hydro_update", "segment", False), (pf.SHAPES[3], "hydro_update", "line", False),
           (pf.SHAPES[4], "loop", "segment", False), (pf.SHAPES[5], "hydro_update", "line", False), (pf.SHAPES[6], "loop", "line", False),
           (pf.SHAPES[1], "loop", "line", True)]


@pytest.mark.parametrize("spec,forms,mode,bright", R_CASES,
                         ids=["%s-%s-%s%s" % (pf.shape_id(c[0]), c[1], c[2], "-bright" if c[3] else "") for c in R_CASES])
def test_resident_phase_equals_the_array_route(spec, forms, mode, bright):
    """2. Simulation.rad_phase(full=True) against compat.rad_phase on the downloaded state and Simulation.neighbors(): every
    stage output, every written array and every total with np.array_equal, in both step modes and both column modes, at
    N = 257 and 2049 (more than 16 sources there), K = 7, 40, S = 7, 15, 32, and N = 33 < K; nothing else of the state
    changes; and a second phase on the state the first left equals its array route again.  The bright case moves the
    velocities."""
    sim, f = rad_prepared(spec, forms, bright=bright)
    res, st, after = assert_equals_array_route(sim, f, mode)
    print(pf.shape_id(spec), forms, mode, {k_: v for k_, v in res.items() if not isinstance(v, np.ndarray)}, sim.radphase_timing())
    assert not res["skipped"]
    assert spec[0] < 2049 or len(f["source_ids"]) > 16
    assert not same(after["E_internal"], st["E_internal"]) and not same(after["T"], st["T"]) and np.any(res["frac_destroyed"] > 0)
    assert not bright or np.max(np.abs(after["velocities"] - st["velocities"])) > 1e-6 * np.max(np.abs(st["velocities"]))
    assert_equals_array_route(sim, f, mode)


@pytest.mark.parametrize("forms", ["loop", "hydro_update"])
def test_next_step_reads_what_the_phase_wrote(forms):
    """3. One fused step after a phase against the oracle's step from the downloaded state; the same oracle step fed the
    E_internal, T, velocities or mu_array from before the phase fails the comparison - a missing write-back would show."""
    spec = pf.SHAPES[1]
    sim, f = rad_prepared(spec, forms, bright=True)
    n, K = spec[0], spec[1]
    b_st, b_comp = sim.download(), sim.download_composition()
    resident(sim, f, full=False)
    st, comp = sim.download(), sim.download_composition()
    s1 = dict(points=st["points"], velocities=st["velocities"], total_accel=st["total_accel"], E_internal=st["E_internal"], T=st["T"],
              particle_type=f["particle_type"], **comp)
    case = (forms, "cloud", n, K)
    sim.step(1, fixed_dt=f["fixed_dt"])
    got = sim.download()
    olds = dict(E_internal=b_st["E_internal"], T=b_st["T"], velocities=b_st["velocities"], mu_array=b_comp["mu_array"])
    with np.errstate(all="ignore"):
        ref = oracle_step(case, s1, f["d"], False, f["fixed_dt"])
        old = {k_: oracle_step(case, dict(s1, **{k_: v}), f["d"], False, f["fixed_dt"]) for k_, v in olds.items()}
    R0, V0 = np.max(np.abs(f["points"])), np.max(np.abs(ref["velocities"]))

    def meets(o):
        fin = np.isfinite(o["E_internal"]) & np.isfinite(got["E_internal"])
        return (np.max(np.abs(got["points"] - o["points"])) <= 1e-12 * R0 and np.max(np.abs(got["velocities"] - o["velocities"])) <= 1e-10 * V0
                and np.allclose(got["E_internal"][fin], o["E_internal"][fin], rtol=1e-9, atol=0)
                and np.allclose(got["T"][fin], o["T"][fin], rtol=1e-9, atol=0))
    print(forms, "x err %.3g, v err %.3g" % (np.max(np.abs(got["points"] - ref["points"])) / R0,
                                              np.max(np.abs(got["velocities"] - ref["velocities"])) / V0))
    assert meets(ref)
    np.testing.assert_allclose(got["sizes"], ref["sizes"], rtol=1e-9)
    np.testing.assert_allclose(got["densities"], ref["densities"], rtol=1e-9)
    for name, o in old.items():
        assert not meets(o), "the oracle step fed the pre-phase %s still meets the library's step" % name


def test_a_whole_pass_of_the_loop_twice():
    """4. rad_phase -> dust_phase -> step, twice on one Simulation: each phase equals its array route on the state
    downloaded just before it."""
    spec = pf.SHAPES[1]
    sim, f = rad_prepared(spec, "loop")
    for _ in range(2):
        assert_equals_array_route(sim, f, "line")
        st, nb, comp = sim.download(), sim.neighbors(), sim.download_composition()
        arr = nsc.dust_phase(st["points"], st["velocities"], nb, comp["mass"], comp["f_un"], comp["mu_array"], st["sizes"], st["T"],
                             f["particle_type"], d=f["d"], dt=f["dt"], guard="fraction", **pf.tables(f))
        sim.dust_phase(f["dt"], f["d"], guard="fraction", **pf.tables(f))
        after = sim.download_composition()
        for name, want in zip(("mass", "f_un", "mu_array", "gamma_array"), arr[:4]):
            assert same(after[name], want), name
        sim.step(1, fixed_dt=f["fixed_dt"])
        assert np.all(np.isfinite(sim.download()["points"]))


def test_resident_refusals_and_the_skipped_block():
    """5. Refused before the first step, in incremental mode, after a compat.density on the same context, without a
    composition, and with drag but no tables (the C entry itself) - the state unchanged each time; no star: skipped, the
    state bit-identical; zero targets and N <= K run (the latter among the cases of test 2)."""
    from sph_code_amd._lib import dp, ip
    from sph_code_amd.sim import Simulation
    import ctypes as C
    spec = pf.SHAPES[1]
    f = rad_set(spec)
    K, s0 = spec[1], pf.sim_state(f)

    def state_of(sim):
        a, st, comp = finals_of(sim)
        return dict(a, points=st["points"], mass=comp["mass"])

    def refused(sim, exc, words):
        before = state_of(sim)
        with pytest.raises(exc, match=words):
            resident(sim, f, full=False)
        after = state_of(sim)
        assert all(same(before[k_], after[k_]) for k_ in before)

    refused(Simulation(s0, n_neigh=K, with_species=True), RuntimeError, "before the first sphx_step")
    sim = Simulation(s0, n_neigh=K, with_species=True, incremental=True)
    sim.step(1, fixed_dt=f["fixed_dt"])
    refused(sim, RuntimeError, "incremental")
    sim = Simulation(s0, n_neigh=K, with_species=False)
    sim.step(1, fixed_dt=f["fixed_dt"])
    refused(sim, RuntimeError, "no composition")
    sim = Simulation(s0, n_neigh=K, with_species=True, ctx=nsc.context())
    sim.step(1, fixed_dt=f["fixed_dt"])
    nsc.density(f["points"], f["mass"], f["particle_type"], f["neighbor"], d=f["d"])
    refused(sim, RuntimeError, "list is gone")
    # drag on, the two per-species tables missing: the C entry itself (Simulation always passes them)
    sim, _ = rad_prepared(spec, "loop", with_drag=True)
    before = state_of(sim)
    t = f["tables"]
    c = sim.ctx
    skipped = C.c_int(0)
    rc = c.lib.sphx_state_rad_phase(c.h, PHASE_DT, f["d"], len(f["source_ids"]), ip(f["source_ids"]), dp(f["luminosities"]),
                                    len(f["target_ids"]), ip(f["target_ids"]), dp(f["frac_dest"]), f["ppj"], dp(t["mu_specie"]), dp(t["gamma"]),
                                    dp(t["cross_sections"]), dp(t["driver_cross"]), nsc.amu, nsc.t_cmb, T_MAX, 4.0 * PHASE_DT, nsc.sb, nsc.k,
                                    nsc.m_h, 0, None, None, None, None, None, None, None, None, None, None, None, None, None, None, None,
                                    C.byref(skipped))
    assert rc == -1 and b"grain_mass" in c.lib.sphx_last_error(c.h)
    after = state_of(sim)
    assert all(same(before[k_], after[k_]) for k_ in before)
    res, _, _ = assert_equals_array_route(sim, f, "line")             # ... and with them it runs, and refreshes the coefficients
    fu = sim.download_composition()["f_un"]
    mgm, mcs = sim.download_drag()
    assert np.array_equal(mgm, np.sum(nsc.grain_mass() * fu, axis=1)) and np.array_equal(mcs, np.sum(nsc.sigma_effective() * fu, axis=1))
    # no star: the driver skips the block
    dark = dict(s0, particle_type=np.where(s0["particle_type"] == 1, 0.0, s0["particle_type"]))
    sim = Simulation(dark, n_neigh=K, with_species=True)
    sim.step(1, fixed_dt=f["fixed_dt"])
    before = state_of(sim)
    assert resident(sim, f, full=False) == dict(skipped=True)
    after = state_of(sim)
    assert all(same(before[k_], after[k_]) for k_ in before)
    # zero targets
    sim, _ = rad_prepared(spec, "hydro_update")
    g = dict(f, target_ids=np.zeros(0, np.int64))
    assert_equals_array_route(sim, g, "line")


def test_side_calls_between_the_phase_and_the_step():
    """6. sample, rad_transfer and rad_cooling called between a rad_phase and the step give the bits of their first
    calls, and the step that follows is the step of a twin Simulation that made none of them."""
    spec = pf.SHAPES[0]
    sim, f = rad_prepared(spec, "hydro_update")
    twin, _ = rad_prepared(spec, "hydro_update")
    resident(sim, f, full=False)
    resident(twin, f, full=False)
    timing = sim.radphase_timing()
    st, comp = sim.download(), sim.download_composition()
    q = st["points"][:50] + 1e13
    cross = nsc.cross_array_of(comp["f_un"])
    src, dst = st["points"][f["source_ids"]], st["points"][f["target_ids"]]
    first = (sim.sample(q, f["d"]), sim.rad_transfer(src, f["luminosities"], dst, cross, PHASE_DT),
             nsc.rad_cooling(st["points"], f["particle_type"], comp["mass"], st["sizes"], cross, comp["f_un"], sim.neighbors(), comp["mu_array"],
                             st["T"], PHASE_DT, d=f["d"]))
    again = (sim.sample(q, f["d"]), sim.rad_transfer(src, f["luminosities"], dst, cross, PHASE_DT),
             nsc.rad_cooling(st["points"], f["particle_type"], comp["mass"], st["sizes"], cross, comp["f_un"], sim.neighbors(), comp["mu_array"],
                             st["T"], PHASE_DT, d=f["d"]))
    assert all(same(first[0][k_], again[0][k_]) for k_ in first[0])
    assert all(same(a, b) for a, b in zip(first[1], again[1])) and all(same(a, b) for a, b in zip(first[2], again[2]))
    assert sim.radphase_timing() == timing and sim.rad_timing()["columns"] > 0
    sim.step(1, fixed_dt=f["fixed_dt"])
    twin.step(1, fixed_dt=f["fixed_dt"])
    a, b = sim.download(), twin.download()
    assert all(same(a[k_], b[k_]) for k_ in a)
