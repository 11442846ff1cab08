"""GPU checks of the radiative transfer (nsc:922-965; include/sphx.h sphx_rad_columns, sphx_rad_transfer,
sphx_state_rad_transfer) against the reference's own captured results (tests/golden/rad_*.npz) and the NumPy
restatement tests/rad_oracle.py, to the bounds that module derives: 1e-12 sum|term| for a column, and that same 1e-12
propagated to first order through lum_factor, the exponent and the sums over the sources.  No element is left out of any
comparison; every comparison first checks that no (particle, ray) pair of its inputs sits on a column's edge."""
import ctypes
import os
import re

import numpy as np
import pytest

import rad_fixture
import rad_oracle
from conftest import ROOT

pytestmark = pytest.mark.gpu

OUT = rad_oracle.OUTPUTS


def layout():
    """The kernels' layout constants, as include/sphx.h documents them."""
    src = open(os.path.join(ROOT, "include", "sphx.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define\s+SPHX_RAD_(TILE|WG_RAYS|SRC_CHUNK)\s+(\d+)", src)}


def gpu_transfer(args, mode="line"):
    import sph_code_amd.compat as nsc
    return dict(zip(OUT, nsc.rad_transfer(*args, mode=mode, full=True)))


def check(got, ref, bounds, what):
    assert bounds["margin"] > rad_fixture.MIN_MARGIN, (what, bounds["margin"])
    for nm in OUT:
        print(what, nm, "worst |diff| / bound %.3g" % rad_oracle.worst_ratio(got[nm], ref[nm], bounds[nm + "_bound"]))
    for nm in OUT:
        rad_oracle.assert_within(nm, got[nm], ref[nm], bounds[nm + "_bound"], what)


@pytest.mark.parametrize("mode", rad_oracle.MODES)
@pytest.mark.parametrize("case", rad_fixture.CASES)
def test_fixture(case, mode):
    """Line mode against the reference's captured values, segment mode against the restatement; the bounds are the
    restatement's in both."""
    f = rad_fixture.load(case)
    o = rad_fixture.oracle(case, mode)
    ref = {nm: f["ref_" + nm] for nm in OUT} if mode == "line" else o
    got = gpu_transfer(rad_fixture.transfer_args(f), mode)
    check(got, ref, o, "%s %s" % (case, mode))
    if mode == "segment":
        assert np.any(got["blocked"] < rad_fixture.oracle(case, "line")["blocked"])


def subset_args(f, idx, sources=None, luminosities=None, targets=None):
    src = f["sources"] if sources is None else sources
    return (f["positions"][idx], f["ptypes"][idx], f["masses"][idx], f["sizes"][idx], f["cross_array"][idx],
            f["mu_array"][idx], src, f["luminosities"] if luminosities is None else luminosities,
            f["targets"] if targets is None else targets, f["dt"])


def seeded_subset(f, n, seed=11):
    """n particles of the fixture in a seeded order that starts with a gas particle (min(sizes over gas) must exist)."""
    rs = np.random.RandomState(seed)
    idx = rs.permutation(f["positions"].shape[0])
    first = int(np.nonzero(f["ptypes"][idx] == 0)[0][0])
    idx[[0, first]] = idx[[first, 0]]
    return idx[:n]


def particle_counts():
    t = layout()["TILE"]
    return [1, 63, 64, 65, t - 1, t + 1, 2048]


@pytest.mark.parametrize("n", particle_counts())
def test_particle_counts_around_the_tile(n):
    """N around the wave and the LDS tile, and N = 2048: 8 tiles under 84 rays, the particle range split 8 ways."""
    import sph_code_amd.compat as nsc
    f = rad_fixture.load("sphere_dust_n2048_k40")
    args = subset_args(f, seeded_subset(f, n))
    for mode in rad_oracle.MODES:
        o = rad_oracle.transfer(*args, mode=mode, **rad_fixture.constants(f))
        check(gpu_transfer(args, mode), o, o, "n=%d %s" % (n, mode))
        blocked, sd = nsc.rad_columns(args[0], args[3], args[2], args[5], args[4], args[6], args[8], mode=mode)
        rad_oracle.assert_within("blocked", blocked, o["blocked"], o["blocked_bound"], "rad_columns n=%d" % n)
        rad_oracle.assert_within("star_distance", sd, o["star_distance"], o["star_distance_bound"], "rad_columns n=%d" % n)


def ray_shapes():
    L = layout()
    return [(1, 1), (7, 9), (5, 13), (1, L["WG_RAYS"] + 1), (L["SRC_CHUNK"] + 1, 3)]


@pytest.mark.parametrize("shape", ray_shapes())
def test_ray_counts_around_the_workgroup(shape):
    """R = 1, 63, 65, one more than a workgroup's rays; n_src one more than the deposit kernel's source chunk."""
    n_src, n_dst = shape
    f = rad_fixture.load("condensed_n1024_k40")
    rs = np.random.RandomState(100 * n_src + n_dst)
    n = f["positions"].shape[0]
    src = f["positions"][rs.choice(n, n_src, replace=False)].copy()
    dst = f["positions"][rs.choice(n, n_dst, replace=False)].copy()
    lum = 10.0 ** rs.uniform(-1.0, 4.0, n_src)
    args = subset_args(f, np.arange(n), src, lum, dst)
    mode = "segment" if n_src == 5 else "line"
    o = rad_oracle.transfer(*args, mode=mode, **rad_fixture.constants(f))
    check(gpu_transfer(args, mode), o, o, "rays %dx%d" % shape)


def test_three_or_more_particle_chunks():
    """The chunking the header documents: 2048 particles are 8 tiles; one ray tile leaves min(2048, 8) = 8 chunks."""
    L = layout()
    f = rad_fixture.load("sphere_dust_n2048_k40")
    n, R = f["positions"].shape[0], f["sources"].shape[0] * f["targets"].shape[0]
    ray_tiles = -(-R // L["WG_RAYS"])
    tiles = -(-n // L["TILE"])
    assert min(-(-2048 // ray_tiles), tiles) >= 3
    # (test_fixture and test_particle_counts_around_the_tile[2048] run exactly this shape against the yardstick)


def test_two_calls_give_identical_bits():
    f = rad_fixture.load("sphere_dust_n2048_k40")
    for mode in rad_oracle.MODES:
        a, b = gpu_transfer(rad_fixture.transfer_args(f), mode), gpu_transfer(rad_fixture.transfer_args(f), mode)
        for nm in OUT:
            assert np.array_equal(a[nm], b[nm], equal_nan=True), (mode, nm)


def test_permuting_sources_and_targets():
    f = rad_fixture.load("sphere_dust_n2048_k40")
    o = rad_fixture.oracle("sphere_dust_n2048_k40", "line")
    base = gpu_transfer(rad_fixture.transfer_args(f))
    rs = np.random.RandomState(3)
    ps, pq = rs.permutation(f["sources"].shape[0]), rs.permutation(f["targets"].shape[0])
    args = subset_args(f, np.arange(f["positions"].shape[0]), f["sources"][ps], f["luminosities"][ps], f["targets"][pq])
    got = gpu_transfer(args)
    assert np.array_equal(got["blocked"], base["blocked"][ps][:, pq])
    assert np.array_equal(got["star_distance"], base["star_distance"][ps][:, pq])
    assert np.array_equal(got["extinction"], base["extinction"])
    # the sums over s and q run in another order: within the bound of the yardstick, not bit for bit
    for nm in ("lf2", "momentum"):
        rad_oracle.assert_within(nm, got[nm], o[nm], o[nm + "_bound"], "permuted")
    rad_oracle.assert_within("lum_factor", got["lum_factor"], o["lum_factor"][ps], o["lum_factor_bound"][ps], "permuted")


def test_edge_semantics():
    import sph_code_amd.compat as nsc
    f = rad_fixture.load("condensed_n1024_k40")
    idx = seeded_subset(f, 300)
    G = int(np.count_nonzero(f["ptypes"][idx] != 1))
    # a degenerate ray: column 0, distance 0, and its source's lum_factor zeroed through nan_to_num
    t = f["targets"].copy()
    t[2] = f["sources"][1]
    args = subset_args(f, idx, targets=t)
    o = rad_oracle.transfer(*args, **rad_fixture.constants(f))
    got = gpu_transfer(args)
    check(got, o, o, "degenerate ray")
    assert got["blocked"][1, 2] == 0.0 and got["star_distance"][1, 2] == 0.0 and np.all(got["lum_factor"][1] == 0.0)
    assert np.any(got["lum_factor"][0] > 0.0)
    # no targets: lum_factor = 0, the deposition unattenuated
    args = subset_args(f, idx, targets=np.zeros((0, 3)))
    o = rad_oracle.transfer(*args, **rad_fixture.constants(f))
    got = gpu_transfer(args)
    assert got["blocked"].shape == (f["sources"].shape[0], 0) and np.all(got["lum_factor"] == 0.0)
    check(got, o, o, "no targets")
    # no sources: zeros
    args = subset_args(f, idx, sources=np.zeros((0, 3)), luminosities=np.zeros(0))
    o = rad_oracle.transfer(*args, **rad_fixture.constants(f))
    got = gpu_transfer(args)
    assert got["lum_factor"].shape == (0, G) and np.all(got["lf2"] == 0.0) and np.all(got["momentum"] == 0.0)
    check(got, o, o, "no sources")
    # no gas: SPHX_E_ARG
    pt = f["ptypes"][idx].copy()
    pt[pt == 0] = 2.0
    bad = list(subset_args(f, idx))
    bad[1] = pt
    with pytest.raises(ValueError, match="ptypes == 0"):
        nsc.rad_transfer(*bad)
    with pytest.raises(ValueError):
        nsc.rad_transfer(*subset_args(f, idx), mode="ray")


def test_status_codes_of_the_c_abi():
    import sph_code_amd.compat as nsc
    from sph_code_amd._lib import dp
    f = rad_fixture.load("condensed_n1024_k40")
    c = nsc.context()
    n = 64
    pos, pt, m, h = (np.ascontiguousarray(f[k][:n]) for k in ("positions", "ptypes", "masses", "sizes"))
    cr, mu = np.ascontiguousarray(f["cross_array"][:n]), np.ascontiguousarray(f["mu_array"][:n])
    src, dst, L = f["sources"], f["targets"], f["luminosities"]
    ns, nd = src.shape[0], dst.shape[0]
    G = int(np.count_nonzero(pt != 1))
    sentinel = np.full((ns, nd), -7.0)

    def columns(n_=n, ns_=ns, nd_=nd, mode=0, pos_=pos, out=sentinel, src_=src):
        return c.lib.sphx_rad_columns(c.h, n_, dp(pos_), dp(h), dp(m), dp(mu), dp(cr), ns_, dp(src_), nd_, dp(dst), mode, dp(out), None)

    def transfer(n_=n, ns_=ns, nd_=nd, mode=0, pt_=pt, L_=L, lf2=None):
        return c.lib.sphx_rad_transfer(c.h, n_, dp(pos), dp(pt_), dp(m), dp(h), dp(cr), dp(mu), ns_, dp(src), dp(L_), nd_, dp(dst),
                                       1.0, mode, dp(lf2), None, None, None, None, None)

    assert columns(ns_=0) == 0 and columns(nd_=0) == 0 and np.all(sentinel == -7.0)      # zero-size: nothing written
    for rc in (columns(n_=-1), columns(ns_=-1), columns(nd_=-1), columns(mode=2), columns(mode=-1), columns(pos_=None),
               columns(out=None), columns(src_=None), transfer(n_=-1), transfer(ns_=-1), transfer(nd_=-1), transfer(mode=5),
               transfer(pt_=None), transfer(L_=None), transfer(pt_=np.full(n, 2.0))):
        assert rc == -1, rc                                                              # SPHX_E_ARG
    assert b"ptypes == 0" in c.lib.sphx_last_error(c.h)
    assert columns() == 0 and np.all(sentinel >= 0.0)
    lf2 = np.full(G, -1.0)
    assert transfer(lf2=lf2) == 0 and np.all(lf2 >= 0.0)                                  # every other output NULL
    ms = np.zeros(4)
    assert c.lib.sphx_rad_last_timing(c.h, dp(ms)) == 0 and np.all(ms >= 0.0) and ms[1] > 0.0
    assert c.lib.sphx_rad_last_timing(c.h, None) == -1
    k = c.constants()
    assert k.solar_luminosity == 3.846e26 and k.c == 299792458.0


def test_resident_state_matches_compat_and_leaves_the_loop_alone():
    import sph_code_amd.compat as nsc
    from sph_code_amd import ics
    from sph_code_amd.sim import Simulation
    s = dict(ics.dusty_sphere(6000, dust_frac=0.1))
    n = s["points"].shape[0]
    rs = np.random.RandomState(9)
    pt = np.array(s["particle_type"], dtype=np.float64)
    mass = np.array(s["mass"], dtype=np.float64)
    stars = rs.choice(np.nonzero(pt == 0)[0], 5, replace=False)
    pt[stars] = 1.0
    mass[stars] *= 50.0
    s["particle_type"], s["mass"] = pt, mass
    cross = 10.0 ** rs.uniform(-25.0, -21.0, n)
    lum = 10.0 ** rs.uniform(0.0, 4.0, 5)
    sim, twin = Simulation(s, n_neigh=40), Simulation(s, n_neigh=40)
    with pytest.raises(RuntimeError, match="-4"):                 # SPHX_E_STATE: sizes do not exist before the first step
        sim.rad_transfer(s["points"][stars], lum, s["points"][:9], cross, 1.0)
    sim.step(2)
    twin.step(2)
    st = sim.download()
    src = st["points"][stars].copy()
    dst = st["points"][rs.choice(np.nonzero(pt != 1)[0], 21, replace=False)].copy()
    dt = st["dt"]
    for mode in rad_oracle.MODES:
        got = sim.rad_transfer(src, lum, dst, cross, dt, mode=mode, full=True)
        ref = nsc.rad_transfer(st["points"], pt, mass, st["sizes"], cross, s["mu_array"], src, lum, dst, dt, mode=mode, full=True)
        for nm, a, b in zip(OUT, got, ref):
            assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), (mode, nm)
        assert np.count_nonzero(got[3]) > 50 and np.all(np.isfinite(got[0]))
    # a third step after the call: the bits of a twin that never made it
    sim.step(1)
    twin.step(1)
    a, b = sim.download(), twin.download()
    for key in ("points", "velocities", "total_accel", "E_internal", "T", "sizes", "densities", "num_densities",
                "visc_heat", "pressure"):
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    assert a["dt"] == b["dt"]
