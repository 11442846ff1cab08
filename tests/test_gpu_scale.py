"""GPU tests (-m gpu) of the adaptive length scale and sizes, code_running.py:493-540: compat.length_scale and
compat.adapt_sizes (include/sphx.h sphx_length_scale, sphx_adapt_sizes) against the NumPy restatement
tests/scale_oracle.py, and Simulation.length_scale (sphx_state_length_scale) against the two array calls on the downloaded
state.

Selection: n_slow, n_nan, lo, a, b, max_dist and d BIT FOR BIT.  Adaptation: the reverse counts, num_nontrivial and the
four counts EXACT; the sizes bit for bit wherever new_smoothing is exactly 1 or 1.1, the row is dust or a star, or there
is no densities_0; elsewhere within EXP_TOL relative, which is the device exp against NumPy's and nothing else (the rest
of drv:533-537 is separately rounded arithmetic on both sides).  EXP_TOL follows the rule of DESIGN 5.18: twice the
largest relative deviation of the device's new_smoothing from the restatement's measured on these inputs on an MI355X
(test_sizes_against_the_restatement prints it), rounded up to a power of two, at most the 16 ulp that
tests/test_gpu_cool.py grants a transcendental coefficient.  MEASURED: 2.22e-16 = 1.00 ulp (MEASURED_EXP_DEV; the test fails
if a run exceeds it, and the figure then has to be measured again).  CHOSEN: 2 ulp = 2^-51 (EXP_TOL).  No row is exempt: a
row the cap drv:537 flips is within that tolerance of d on both sides.

Resident: every comparison is bit for bit between the resident call and the array route on identical inputs, or between
twin Simulations."""
import numpy as np
import pytest

import phase_fixture as pf
import scale_oracle as so

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -52
MEASURED_EXP_DEV = 1.0 * ULP         # the largest |device - NumPy| / NumPy of new_smoothing over the rows of this file, on an MI355X
EXP_TOL = 2.0 * ULP                  # twice that, a power of two, <= 16 ulp
assert MEASURED_EXP_DEV * 2.0 <= EXP_TOL <= 16.0 * ULP
N_INT = 40
RAISE = 8.0
SEL_KEYS_INT = ("n_slow", "n_nan", "lo")
SEL_KEYS_F64 = ("a", "b", "max_dist", "d")


@pytest.fixture(scope="module")
def nsc():
    import sph_code_amd.compat as nsc_mod
    nsc_mod.context()
    return nsc_mod


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


# ---------------------------------------------------------------------------------------------------------------------
# selection
# ---------------------------------------------------------------------------------------------------------------------
def on_the_x_axis(x, fast=None):
    """Rows at (x, 0, 0) - dist_sq = x * x, controlled - at rest, the rows `fast` at 100 km/s."""
    x = np.asarray(x, dtype=np.float64)
    pts = np.zeros((x.shape[0], 3))
    pts[:, 0] = x
    vel = np.zeros((x.shape[0], 3))
    if fast is not None:
        vel[np.asarray(fast), 1] = 1e5
    return pts, vel


def cloud(n, seed):
    rs = np.random.RandomState(seed)
    pts = rs.normal(size=(n, 3)) * 3e16
    vel = rs.normal(size=(n, 3)) * 3e4
    vel[rs.rand(n) < 0.1] *= 10.0
    return pts, vel


def check_selection(nsc, pts, vel, what):
    with np.errstate(all="ignore"):
        ref = so.length_scale(pts, vel, N_INT)
    got = nsc.length_scale(pts, vel, N_INT, full=True)
    print(what, got, nsc.scale_last_timing())
    for key in SEL_KEYS_INT:
        assert got[key] == ref[key], (what, key, got[key], ref[key])
    for key in SEL_KEYS_F64:
        assert so.same_bits(got[key], ref[key]), (what, key, got[key], ref[key])
    assert so.same_bits(nsc.length_scale(pts, vel, N_INT), ref["d"])
    return got


@pytest.mark.parametrize("n", [1, 2, 11, 255, 256, 257, 2049, 20011])
def test_selection_on_clouds(nsc, n):
    pts, vel = cloud(n, 100 + n)
    if n <= 2:
        vel[:] = 0.0                                  # (every row slow)
    got = check_selection(nsc, pts, vel, "cloud n=%d" % n)
    assert got["n_nan"] == 0 and np.isfinite(got["d"]) and got["d"] > 0


@pytest.mark.parametrize("M", [1, 2])
def test_few_slow_rows_inside_a_larger_set(nsc, M):
    pts, vel = cloud(300, 7)
    vel[:] = 1e5
    vel[[17, 255][:M]] = 0.0
    assert check_selection(nsc, pts, vel, "M=%d of 300" % M)["n_slow"] == M


def test_all_rows_fast_is_refused(nsc):
    pts, vel = cloud(300, 8)
    vel[:, 0] = 1e5
    with pytest.raises(ValueError, match="slower"):
        nsc.length_scale(pts, vel, N_INT)


def chain(start, count):
    out = [np.float64(start)]
    for _ in range(count - 1):
        out.append(np.nextafter(out[-1], np.inf))
    return np.array(out)


def test_keys_at_the_histogram_edges(nsc):
    """Every level of the radix selection decides something in one of these."""
    rs = np.random.RandomState(3)
    # every key equal
    check_selection(nsc, *on_the_x_axis(np.full(100, 3.0)), "all equal")
    # keys that differ only in their lowest byte: x * x over a chain of adjacent x from 1.5 (2.25: a zero low byte)
    x = chain(1.5, 100)
    sq = np.unique((x * x).view(np.uint64))
    assert sq.shape[0] > 50 and np.all(sq >> np.uint64(8) == sq[0] >> np.uint64(8))
    check_selection(nsc, *on_the_x_axis(rs.permutation(x)), "lowest byte")
    # ... and only in the lowest two bytes (the last level but one decides)
    x = 1.5 + np.arange(100) * 2.0 ** -44
    check_selection(nsc, *on_the_x_axis(rs.permutation(x)), "two low bytes")
    # the whole exponent range, 1e-300 .. 1e300 in dist_sq
    x = 10.0 ** rs.uniform(-150.0, 150.0, 4097)
    got = check_selection(nsc, *on_the_x_axis(x), "exponent range")
    assert got["a"] != got["b"]
    # rank lo the last row of a top-level bin (keys below 2.0: top byte 0x3F), rank hi in the next (2.25: 0x40); M = 11: lo = 9
    x = np.concatenate((np.linspace(0.1, 1.4, 10), [1.5]))
    got = check_selection(nsc, *on_the_x_axis(rs.permutation(x)), "bin edge")
    assert got["lo"] == 9 and got["a"] < 2.0 < got["b"] == 2.25
    # lo and hi among duplicates (M = 21: lo = 18, hi = 19) ...
    got = check_selection(nsc, *on_the_x_axis(rs.permutation([1.0] * 5 + [2.0] * 16)), "duplicates")
    assert got["lo"] == 18 and got["a"] == got["b"] == 4.0
    # ... and lo the last of its duplicates, hi the next distinct key
    got = check_selection(nsc, *on_the_x_axis(rs.permutation([1.0] * 19 + [2.0] * 2)), "last duplicate")
    assert got["a"] == 1.0 and got["b"] == 4.0
    # the same with fast rows below, between and above (they are not counted)
    x = np.concatenate(([1.0] * 19 + [2.0] * 2, [0.5, 1.5, 1.5, 9.0]))
    got = check_selection(nsc, *on_the_x_axis(x, fast=[21, 22, 23, 24]), "fast rows between")
    assert got["n_slow"] == 21 and got["a"] == 1.0 and got["b"] == 4.0


def test_inf_and_nan(nsc):
    rs = np.random.RandomState(5)
    x = 10.0 ** rs.uniform(-3.0, 3.0, 257)
    # inf positions, and positions whose square overflows, among the slow rows: the top tenth
    xi = x.copy()
    xi[:20] = np.inf
    xi[20:40] = 1e200
    got = check_selection(nsc, *on_the_x_axis(xi), "inf")
    assert got["n_nan"] == 0 and np.isinf(got["a"]) and np.isinf(got["b"])
    # one NaN position among the slow rows: NaN result, n_nan = 1, as np.percentile gives
    xn = x.copy()
    xn[100] = np.nan
    got = check_selection(nsc, *on_the_x_axis(xn), "nan")
    assert got["n_nan"] == 1 and np.isnan(got["max_dist"]) and np.isnan(got["d"]) and got["n_slow"] == 257
    # a NaN position in a FAST row is not met
    got = check_selection(nsc, *on_the_x_axis(xn, fast=[100]), "nan in a fast row")
    assert got["n_nan"] == 0 and got["n_slow"] == 256 and np.isfinite(got["d"])
    # NaN velocities: excluded (a NaN speed is not slow)
    pts, vel = on_the_x_axis(x)
    vel[::7, 2] = np.nan
    got = check_selection(nsc, pts, vel, "nan velocities")
    assert got["n_slow"] == 257 - len(range(0, 257, 7))


def test_same_bits_twice_and_in_any_row_order(nsc):
    pts, vel = cloud(20011, 9)
    first = nsc.length_scale(pts, vel, N_INT, full=True)
    assert nsc.length_scale(pts, vel, N_INT, full=True) == first
    p = np.random.RandomState(10).permutation(pts.shape[0])
    assert nsc.length_scale(pts[p], vel[p], N_INT, full=True) == first


# ---------------------------------------------------------------------------------------------------------------------
# adaptation
# ---------------------------------------------------------------------------------------------------------------------
def adapt_case(n, K, seed, kind="random"):
    """-> dict of adapt_sizes' arguments.  kind: random (missing entries among them), hub (row 0 listed by every row), self
    (rows listed only by themselves: the bonus rows)."""
    rs = np.random.RandomState(seed)
    nb = rs.randint(0, n, size=(n, K)).astype(np.int64)
    nb[:, 0] = np.arange(n)
    nb[rs.rand(n, K) < 0.1] = n                                   # missing, compat.neighbors' convention
    nb[rs.rand(n, K) < 0.02] = -1                                 # ... and other entries outside [0, n)
    if n <= K:
        nb[:, n:] = n
    if kind == "hub" and K > 1:
        nb[:, K - 1] = 0
    if kind == "self":
        nb[:] = n
        nb[:, 0] = np.arange(n)
    rho = np.exp(rs.normal(size=n)) * 1e-20
    rho0 = rho * np.exp(0.3 * rs.normal(size=n))
    keep = rs.rand(n) < 0.2
    rho0[keep] = rho[keep]                                        # new_smoothing exactly 1 (or 1.1)
    sizes = np.abs(rs.normal(size=n)) + 0.05
    pt = rs.choice([0.0, 1.0, 2.0], size=n, p=[0.7, 0.1, 0.2])
    d = float(np.percentile(sizes, 70))
    sizes[rs.rand(n) < 0.1] = 3.0 * d                             # above d before the product
    if n >= 8:                                                    # the edge rows, gas
        pt[:8] = 0.0
        rho[0] = 0.0                                              # +inf under the nan_to_num: DBL_MAX, exp = inf, capped
        rho[1] = np.nan                                           # NaN -> 0: new_smoothing 1
        rho0[2] = np.inf                                          # +inf again
        sizes[3] = np.nan                                         # stays NaN
        rho[4], rho0[4] = 0.0, 0.0                                # 0 / 0
        rho[5], rho0[5] = 0.0, -1.0                               # -inf -> -DBL_MAX: exp = 0
        rho0[6] = np.nan
        sizes[7] = np.inf
    return dict(neighbor=nb, densities=rho, densities_0=rho0, sizes=sizes, particle_type=pt, d=d, raise_factor=RAISE)


def check_adapt(nsc, c, with_d0, what):
    """-> the largest relative deviation of the device's new_smoothing from the restatement's over its finite rows."""
    d0 = c["densities_0"] if with_d0 else None
    args = (c["neighbor"], c["densities"], d0, c["sizes"], c["particle_type"], c["d"], c["raise_factor"])
    ref = so.adapt_sizes(*args)
    before = c["sizes"].copy()
    got, info = nsc.adapt_sizes(*args, full=True)
    assert np.array_equal(before, c["sizes"], equal_nan=True)                         # (the caller's array is left alone)
    n = c["sizes"].shape[0]
    nb = c["neighbor"]
    ok = (nb >= 0) & (nb < n)
    assert np.array_equal(info["exp_neighbor_count"], np.bincount(nb[ok], minlength=n))
    assert np.array_equal(info["exp_neighbor_count"], ref["exp_neighbor_count"])
    assert np.array_equal(info["num_nontrivial"], ref["num_nontrivial"])
    assert info["counts"] == ref["counts"], (what, info["counts"], ref["counts"])
    ns_ref, ns = ref["new_smoothing"], info["new_smoothing"]
    exact = (ns_ref == 1.0) | (ns_ref == 1.1) | (c["particle_type"] != 0.0)
    if not with_d0:
        exact[:] = True
    assert so.same_bits(got[exact], ref["sizes"][exact]), what
    assert so.same_bits(ns[(ns_ref == 1.0) | (ns_ref == 1.1)], ns_ref[(ns_ref == 1.0) | (ns_ref == 1.1)]), what
    # the rest: relative, every row; NaN with NaN, inf with inf
    g, r = got[~exact], ref["sizes"][~exact]
    with np.errstate(all="ignore"):
        bad = ~((g == r) | (np.isnan(g) & np.isnan(r)) | (np.abs(g - r) <= EXP_TOL * np.abs(r)))
    assert not bad.any(), (what, int(bad.sum()), g[bad][:4], r[bad][:4])
    fin = np.isfinite(ns_ref) & (ns_ref != 0.0) & np.isfinite(ns)
    dev = float(np.max(np.abs(ns[fin] - ns_ref[fin]) / np.abs(ns_ref[fin]))) if fin.any() else 0.0
    assert same(np.isfinite(ns), np.isfinite(ns_ref))
    assert same(nsc.adapt_sizes(*args), got)
    return dev, info


A_SHAPES = [(257, 1), (257, 7), (2049, 40), (300, 64), (33, 40), (5, 7), (1, 1)]


def test_sizes_against_the_restatement(nsc):
    """Every shape and list kind, with and without densities_0; prints the measured deviation of the device's exp."""
    worst = 0.0
    for n, K in A_SHAPES:
        for kind in ("random", "hub", "self"):
            c = adapt_case(n, K, 1000 * K + n, kind)
            dev, info = check_adapt(nsc, c, True, "n=%d K=%d %s" % (n, K, kind))
            worst = max(worst, dev)
            if kind == "self":
                assert info["counts"]["bonus"] == n and np.all(info["exp_neighbor_count"] == 1)
            if kind == "hub" and K > 1 and n > 1:
                assert info["exp_neighbor_count"][0] >= n
            if n >= 8:
                assert info["counts"]["nan_to_num"] >= 5 and info["counts"]["capped"] > 0
            dev0, info0 = check_adapt(nsc, c, False, "n=%d K=%d %s no densities_0" % (n, K, kind))
            assert dev0 == 0.0 and info0["counts"]["bonus"] == 0 and info0["counts"]["nan_to_num"] == 0
            assert np.all(info0["new_smoothing"] == 1.0)
    print("largest relative deviation of new_smoothing (the device's exp against NumPy's): %.3g = %.2f ulp; EXP_TOL %.3g"
          % (worst, worst / ULP, EXP_TOL))
    assert worst <= MEASURED_EXP_DEV, "the measured deviation stated in this file and in DESIGN 5.18 no longer holds"


def test_a_shorter_densities_0_is_none(nsc):
    c = adapt_case(257, 7, 77)
    a = nsc.adapt_sizes(c["neighbor"], c["densities"], c["densities_0"][:250], c["sizes"], c["particle_type"], c["d"], RAISE)
    b = nsc.adapt_sizes(c["neighbor"], c["densities"], None, c["sizes"], c["particle_type"], c["d"], RAISE)
    assert same(a, b)


@pytest.mark.parametrize("name", ["scale_a", "scale_b"])
def test_the_driver_blocks_fixtures(nsc, name):
    """The array calls against what code_running.py:493-540 itself left (tests/golden/make_golden_scale.py)."""
    from conftest import load_golden
    g = load_golden(name)
    got = nsc.length_scale(g["points"], g["velocities"], int(g["N_INT_PER_PARTICLE"]), full=True)
    assert got["n_slow"] == int(g["out_n_slow"]) and so.same_bits(got["max_dist"], g["out_max_dist"]) and so.same_bits(got["d"], g["out_d"])
    sizes, info = nsc.adapt_sizes(g["neighbor"], g["densities"], g["densities_0"], g["sizes"], g["particle_type"], got["d"],
                                  float(g["raise_factor"]), full=True)
    assert np.array_equal(info["exp_neighbor_count"], g["out_exp_neighbor_count"])
    r = g["out_sizes"]
    with np.errstate(all="ignore"):
        assert np.all((sizes == r) | (np.isnan(sizes) & np.isnan(r)) | (np.abs(sizes - r) <= EXP_TOL * np.abs(r)))
    if name == "scale_b":
        assert so.same_bits(sizes, r)


# ---------------------------------------------------------------------------------------------------------------------
# resident
# ---------------------------------------------------------------------------------------------------------------------
SPHERE = "sphere"
TWO_PHASE = pf.SHAPES[4]                 # n = 2049, K = 40, S = 32
R_CASES = [(SPHERE, "hydro_update"), (TWO_PHASE, "loop")]
STEP_KEYS = ("points", "velocities", "total_accel", "E_internal", "T", "sizes", "densities", "num_densities", "visc_heat", "pressure", "dt")


def the_set(spec):
    return pf.sphere() if spec == SPHERE else pf.state(*spec)


def prepared(spec, forms, steps=1, **kw):
    from sph_code_amd.sim import Simulation
    f = the_set(spec)
    K = f["neighbor"].shape[1]
    mode = dict(forms="loop", d=f["d"]) if forms == "loop" else {}
    sim = Simulation(pf.sim_state(f), n_neigh=K, with_species=True, **mode, **kw)
    for _ in range(steps):
        sim.step(1, fixed_dt=f["fixed_dt"])
    return sim, f


def array_route(nsc, sim, ptype, densities_0):
    """The two array calls on what the Simulation holds -> (length_scale's dict, sizes, adapt_sizes' dict, the download)."""
    st, nb = sim.download(), sim.neighbors()
    ls = nsc.length_scale(st["points"], st["velocities"], N_INT, full=True)
    sizes, info = nsc.adapt_sizes(nb, st["densities"], densities_0, st["sizes"], ptype, ls["d"], RAISE, full=True)
    return ls, sizes, info, st


def assert_resident_equals(res, ls, sizes, info):
    for key in SEL_KEYS_INT:
        assert res[key] == ls[key], key
    for key in SEL_KEYS_F64:
        assert so.same_bits(res[key], ls[key]), (key, res[key], ls[key])
    assert so.same_bits(res["d_dust"], ls["d"] / RAISE ** (1. / 3.))
    assert res["counts"] == info["counts"], (res["counts"], info["counts"])
    assert np.array_equal(res["exp_neighbor_count"], info["exp_neighbor_count"])
    assert so.same_bits(res["sizes"], sizes)


def snapshot(sim):
    st = sim.download()
    st.update(sim.download_composition())
    st["neighbors"] = sim.neighbors()
    return st


def unchanged(a, b):
    return all(same(a[key], b[key]) for key in a)


@pytest.mark.parametrize("spec,forms", R_CASES, ids=["sphere-hydro_update", "two_phase-loop"])
def test_resident_equals_the_array_route(nsc, spec, forms):
    """After one step: the bits of the two array calls with densities_0 = None.  After a second: with the first step's
    downloaded densities.  download() keeps the radii; download_sizes() has the adapted sizes until the next step."""
    sim, f = prepared(spec, forms)
    pt = f["particle_type"]
    with pytest.raises(RuntimeError, match="no adapted sizes"):
        sim.download_sizes()
    ls, sizes, info, st1 = array_route(nsc, sim, pt, None)
    before = snapshot(sim)
    res = sim.length_scale(N_INT, RAISE, full=True)
    print(spec, forms, {k_: v for k_, v in res.items() if not isinstance(v, np.ndarray)}, sim.scale_timing())
    assert_resident_equals(res, ls, sizes, info)
    assert res["counts"]["bonus"] == 0 and res["counts"]["nan_to_num"] == 0 and res["counts"]["missing"] == 0
    assert unchanged(before, snapshot(sim))                                    # (download()["sizes"] among them: still the radii)
    assert so.same_bits(sim.download_sizes(), sizes) and not same(sizes, st1["sizes"])
    assert np.all(sizes[pt == 2.0] == res["d_dust"]) and same(sizes[pt == 1.0], st1["sizes"][pt == 1.0])
    tm = sim.scale_timing()
    assert tuple(tm) == nsc.SCALE_STAGES and all(np.isfinite(v) and v >= 0.0 for v in tm.values()) and sum(tm.values()) > 0.0
    sim.step(1, fixed_dt=f["fixed_dt"])
    with pytest.raises(RuntimeError, match="no adapted sizes"):
        sim.download_sizes()
    ls2, sizes2, info2, st2 = array_route(nsc, sim, pt, st1["densities"])
    res2 = sim.length_scale(N_INT, RAISE, full=True)
    assert_resident_equals(res2, ls2, sizes2, info2)
    assert not np.all(info2["new_smoothing"] == 1.0)
    # apply=False between: the same outputs, nothing kept (densities_0 is still the second step's)
    sim.step(1, fixed_dt=f["fixed_dt"])
    ls3, sizes3, info3, st3 = array_route(nsc, sim, pt, st2["densities"])
    res3 = sim.length_scale(N_INT, RAISE, apply=False, full=True)
    assert_resident_equals(res3, ls3, sizes3, info3)
    with pytest.raises(RuntimeError, match="no adapted sizes"):
        sim.download_sizes()
    assert_resident_equals(sim.length_scale(N_INT, RAISE, full=True), ls3, sizes3, info3)


def test_behind_an_explosion_the_scale_is_one_again(nsc):
    from sph_code_amd.sim import Simulation
    f = dict(the_set(SPHERE))
    pt = f["particle_type"]
    stars = np.concatenate((np.nonzero(pt == 1.0)[0], np.nonzero(pt == 0.0)[0]))[:1].astype(np.int64)
    m = np.array(f["mass"], dtype=np.float64)
    m[stars] = 10.0 * nsc.solar_mass                    # (a progenitor the yield tables know, as tests/test_gpu_explosion.py sets it)
    f["mass"] = m
    sim = Simulation(pf.sim_state(f), n_neigh=f["neighbor"].shape[1], with_species=True, forms="loop", d=f["d"])
    for _ in range(2):
        sim.step(1, fixed_dt=f["fixed_dt"])
    sim.length_scale(N_INT, RAISE)
    pre = sim.download()
    np.random.seed(4242)
    ex = sim.supernova_explosion(stars, float(np.median(pre["sizes"])), nsc.t_cmb, mu_specie=f["mu_specie"], gamma=f["gamma"])
    assert ex["n_dust"] + ex["n_gas"] > 0
    with pytest.raises(RuntimeError, match="no adapted sizes"):
        sim.download_sizes()
    pt_new = sim._ptype.copy()
    # before the next step (densities download as zeros, and are not read) and after it: new_smoothing = 1.
    for stepped in (False, True):
        if stepped:
            sim.step(1, fixed_dt=f["fixed_dt"])
        ls, sizes, info, st = array_route(nsc, sim, pt_new, None)
        res = sim.length_scale(N_INT, RAISE, full=True)
        assert_resident_equals(res, ls, sizes, info)
        assert res["counts"]["bonus"] == 0 and res["sizes"].shape[0] == pt.shape[0] + ex["n_dust"] + ex["n_gas"]


def test_phases_read_the_adapted_sizes(nsc):
    """dust_phase and rad_phase behind length_scale(apply=True) have the bits of the array routes fed download_sizes() and
    the remembered d (d=None); a twin that called length_scale(apply=False), and one that never called it, have today's."""
    import test_gpu_radphase as trp
    spec = TWO_PHASE
    sims = [trp.rad_prepared(spec, "loop")[0] for _ in range(3)]
    f = trp.rad_set(spec)
    sim, twin_off, twin_never = sims
    res = sim.length_scale(N_INT, RAISE)
    off = twin_off.length_scale(N_INT, RAISE, apply=False)
    assert off["d"] == res["d"]
    with pytest.raises(ValueError, match="remembered"):
        twin_off.dust_phase(f["dt"], None, guard="fraction", **pf.tables(f))
    adapted = sim.download_sizes()
    # ---- the radiative phase ----
    st, nb, comp = sim.download(), sim.neighbors(), sim.download_composition()
    want = nsc.rad_phase(st["points"], st["velocities"], nb, comp["mass"], comp["f_un"], comp["mu_array"], adapted, st["T"],
                         st["E_internal"], f["particle_type"], *trp.rad_args(f), trp.PHASE_DT, res["d"], trp.T_MAX, 4.0 * trp.PHASE_DT,
                         full=True, **f["tables"])
    got = sim.rad_phase(trp.PHASE_DT, None, *trp.rad_args(f), trp.T_MAX, 4.0 * trp.PHASE_DT, full=True, **f["tables"])
    for name in sim.RADPHASE_STAGES:
        assert same(got[name], want[7][name]), name
    today = [t.rad_phase(trp.PHASE_DT, f["d"], *trp.rad_args(f), trp.T_MAX, 4.0 * trp.PHASE_DT, full=True, **f["tables"])
             for t in (twin_off, twin_never)]
    for name in sim.RADPHASE_STAGES:
        assert same(today[0][name], today[1][name]), name
    assert not all(same(got[name], today[1][name]) for name in sim.RADPHASE_STAGES)
    assert so.same_bits(sim.download_sizes(), adapted)                           # (a phase leaves them standing)
    # ---- the dust phase ----
    st, nb, comp = sim.download(), sim.neighbors(), sim.download_composition()
    want = nsc.dust_phase(st["points"], st["velocities"], nb, comp["mass"], comp["f_un"], comp["mu_array"], adapted, st["T"],
                          f["particle_type"], d=res["d"], dt=f["dt"], guard="fraction", full=True, **pf.tables(f))
    got = sim.dust_phase(f["dt"], None, guard="fraction", full=True, **pf.tables(f))
    for name in ("density", "mass_chem", "f_un_chem", "frac_destruction", "frac_reuptake"):
        assert same(got[name], want[5][name]), name
    today = [t.dust_phase(f["dt"], f["d"], guard="fraction", full=True, **pf.tables(f)) for t in (twin_off, twin_never)]
    for name in ("density", "mass_chem", "f_un_chem", "frac_destruction", "frac_reuptake"):
        assert same(today[0][name], today[1][name]), name
    a, b = snapshot(twin_off), snapshot(twin_never)
    assert unchanged(a, b)


def test_impulse_and_transfer_read_the_adapted_sizes(nsc):
    """The crossing time of supernova_impulse and rad_transfer take the adapted sizes while they stand."""
    sim, f = prepared(SPHERE, "hydro_update")
    pt = f["particle_type"]
    sim.length_scale(N_INT, RAISE)
    adapted = sim.download_sizes()
    st, nb = sim.download(), sim.neighbors()
    n = pt.shape[0]
    rs = np.random.RandomState(3)
    cross = 10.0 ** rs.uniform(-25.0, -21.0, n)
    src, dst, lum = st["points"][:2].copy(), st["points"][100:103].copy(), np.array([10.0, 100.0])
    comp = sim.download_composition()
    want = nsc.rad_transfer(st["points"], pt, comp["mass"], adapted, cross, comp["mu_array"], src, lum, dst, 1e9)
    got = sim.rad_transfer(src, lum, dst, cross, 1e9)
    for x, y in zip(got, want):
        assert same(x, y)
    star = np.concatenate((np.nonzero(pt == 1.0)[0], np.nonzero(pt == 0.0)[0]))[:1].astype(np.int64)
    ev = sim.supernova_impulse(star)
    v1 = sim.download()["velocities"]
    assert same(ev["ct"], nsc.crossing_time(nb, v1, adapted, pt))


def test_the_next_step_in_hydro_update_mode_is_a_twins(nsc):
    sim, f = prepared(SPHERE, "hydro_update")
    twin, _ = prepared(SPHERE, "hydro_update")
    sim.length_scale(N_INT, RAISE)
    for s in (sim, twin):
        s.step(1, fixed_dt=f["fixed_dt"])
    a, b = sim.download(), twin.download()
    for key in STEP_KEYS:
        assert same(a[key], b[key]), key
    assert np.array_equal(sim.neighbors(), twin.neighbors())


def test_the_next_step_in_loop_mode_uses_the_new_d(nsc):
    sim, f = prepared(TWO_PHASE, "loop")
    twin, _ = prepared(TWO_PHASE, "loop")
    res = sim.length_scale(N_INT, RAISE)
    assert res["d"] != f["d"]
    c = twin.ctx
    c.check(c.lib.sphx_state_set_loop_forms(c.h, 1, res["d"]))
    for s in (sim, twin):
        s.step(1, fixed_dt=f["fixed_dt"])
    a, b = sim.download(), twin.download()
    for key in STEP_KEYS:
        assert same(a[key], b[key]), key
    third, _ = prepared(TWO_PHASE, "loop", steps=2)
    assert not same(third.download()["densities"], a["densities"])              # (d matters to the loop forms)


def test_refused_calls_leave_the_state_untouched(nsc):
    from sph_code_amd.sim import Simulation
    f = the_set(TWO_PHASE)
    K = f["neighbor"].shape[1]
    # before the first step
    sim = Simulation(pf.sim_state(f), n_neigh=K, with_species=True, forms="loop", d=f["d"])
    with pytest.raises(RuntimeError, match="before the first"):
        sim.length_scale(N_INT, RAISE)
    # with incremental search
    inc = Simulation(pf.sim_state(f), n_neigh=K, with_species=True, incremental=True)
    inc.step(1, fixed_dt=f["fixed_dt"])
    with pytest.raises(RuntimeError, match="incremental"):
        inc.length_scale(N_INT, RAISE)
    # a NaN d with apply=True.  (The step's clamp drv:233-238 leaves no NaN position on the device; a negative fill gives
    # a negative volume per row, whose cube root is NaN.)  Also: a q outside [0, 100], no slow row.
    state = pf.sim_state(f)
    sim = Simulation(state, n_neigh=K, with_species=True, forms="loop", d=f["d"])
    sim.step(1, fixed_dt=f["fixed_dt"])
    good = sim.length_scale(N_INT, RAISE)
    kept = sim.download_sizes()
    twin = Simulation(state, n_neigh=K, with_species=True, forms="loop", d=f["d"])
    twin.step(1, fixed_dt=f["fixed_dt"])
    twin.length_scale(N_INT, RAISE)
    before = snapshot(sim)
    with pytest.raises(ValueError, match="qf"):
        sim.length_scale(N_INT, RAISE, q=101.)
    with pytest.raises(ValueError, match="slower"):
        sim.length_scale(N_INT, RAISE, v_max=0.0)
    with pytest.raises(ValueError, match="d is NaN"):
        sim.length_scale(N_INT, RAISE, fill=-1.0)
    assert unchanged(before, snapshot(sim)) and so.same_bits(sim.download_sizes(), kept)
    assert np.isnan(sim.length_scale(N_INT, RAISE, fill=-1.0, apply=False)["d"])
    assert sim._scale_d == good["d"]
    for s in (sim, twin):
        s.step(1, fixed_dt=f["fixed_dt"])
    a, b = sim.download(), twin.download()
    for key in STEP_KEYS:
        assert same(a[key], b[key]), key


def test_the_scale_timer_is_apart_from_the_other_side_calls(nsc):
    """tests/test_gpu_side_calls.py's pattern: a call of one family leaves the other families' timings alone."""
    import test_gpu_side_calls as side
    pts, vel = cloud(2049, 21)
    c = adapt_case(257, 7, 5)

    def timings():
        t = side.timings(nsc)
        t["scale"] = nsc.scale_last_timing()
        return t

    for fam in ("arb", "rad", "cool"):
        side.CALLS[fam](nsc)
    nsc.length_scale(pts, vel, N_INT)
    for fam in ("scale", "rad", "arb", "scale", "cool"):
        before = timings()
        if fam == "scale":
            nsc.length_scale(pts, vel, N_INT)
        else:
            side.CALLS[fam](nsc)
        after = timings()
        assert tuple(after["scale"]) == nsc.SCALE_STAGES
        assert all(np.isfinite(v) and v >= 0.0 for v in after[fam].values()), after[fam]
        for other in after:
            if other != fam:
                assert after[other] == before[other], (fam, other)
    assert sum(nsc.scale_last_timing().values()) > 0.0
    nsc.adapt_sizes(c["neighbor"], c["densities"], c["densities_0"], c["sizes"], c["particle_type"], c["d"], RAISE)
    t = nsc.scale_last_timing()
    assert tuple(t) == nsc.SCALE_STAGES and all(np.isfinite(v) and v >= 0.0 for v in t.values()) and t["reverse_counts"] + t["adapt"] > 0.0
    # a call refused by its argument check keeps the previous timing; one refused behind it (no slow row) zeroes its own
    before = timings()
    with pytest.raises(ValueError):
        nsc.length_scale(pts, vel, N_INT, q=150.)
    assert timings() == before
    with pytest.raises(ValueError):
        nsc.length_scale(pts, vel, N_INT, v_max=0.0)
    after = timings()
    assert all(v == 0.0 for v in after["scale"].values())
    for other in ("arb", "rad", "cool"):
        assert after[other] == before[other]
