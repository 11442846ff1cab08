"""GPU checks of the arbitrary-point samplers (nsc:1422-1527; include/sphx.h sphx_arb_fields, sphx_arb_fields_list,
sphx_state_sample) against the reference's own outputs (tests/golden/arb_*.npz) and the NumPy restatement
tests/arb_oracle.py, to the bounds that module derives.  No point is left out of any comparison."""
import numpy as np
import pytest

import arb_oracle
from conftest import load_golden

pytestmark = pytest.mark.gpu

CASES = ["sphere_dust_n2048_k40", "cube_gas_n2048_k40", "condensed_n1024_k40"]
FIELDS = arb_oracle.FIELDS


def case_inputs(case):
    g, a = load_golden(case), load_golden("arb_" + case)
    kw = dict(points=g["points"], mass=g["mass"], particle_type=g["particle_type"], sizes=g["nb_h"], T=g["T"],
              n_part=a["n_part"], value=a["photoionization"], d=float(g["loop_d"]), m_0=float(g["const_m_0"]))
    return g, a, kw


def rows_of(a, tag):
    rs, mem = a[tag + "_row_start"].astype(np.int64), a[tag + "_members"].astype(np.int64)
    return [mem[rs[j]:rs[j + 1]].tolist() for j in range(len(rs) - 1)]


def gpu_fields(nsc, kw, q, narb, fields=FIELDS, with_stats=True):
    return nsc.arb_fields(kw["points"], q, kw["mass"], kw["particle_type"], narb, sizes=kw.get("sizes"), T=kw.get("T"),
                          N_PART=kw.get("n_part"), photoionization=kw.get("value"), d=kw["d"], fields=fields,
                          with_stats=with_stats)


def oracle_chunked(kw, q, radius, chunk=256):
    """arb_oracle.fields on the brute-force eps = 0 ball, a chunk of points at a time (the pair list of all points at
    once does not fit in memory when R spans the cloud)."""
    parts = []
    for s in range(0, q.shape[0], chunk):
        rs, mem = arb_oracle.brute_ball(kw["points"], q[s:s + chunk], radius)
        parts.append(arb_oracle.fields(arb_points=q[s:s + chunk], row_start=rs, members=mem, **kw))
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def check_against(got, ref_out, bounds, what):
    for name in FIELDS:
        if name in got:
            arb_oracle.assert_within(name, got[name], ref_out[name], bounds[name + "_bound"], what=what)


@pytest.mark.parametrize("case", CASES)
def test_list_form_matches_reference_on_its_own_lists(case):
    import sph_code_amd.compat as nsc
    g, a, kw = case_inputs(case)
    o = arb_oracle.fields(arb_points=a["arb_points"], row_start=a["ref_row_start"], members=a["ref_members"], **kw)
    got = gpu_fields(nsc, kw, a["arb_points"], rows_of(a, "ref"))
    check_against(got, {n: a["ref_" + n] for n in FIELDS}, o, "%s list form" % case)
    assert np.array_equal(got["count"], np.diff(a["ref_row_start"]))
    # the six drop-in functions, with the reference's positional signatures and the module global d
    nsc.d = kw["d"]
    try:
        narb = rows_of(a, "ref")
        p, q, m, t, s, T = kw["points"], a["arb_points"], kw["mass"], kw["particle_type"], kw["sizes"], kw["T"]
        single = {"density": nsc.density_arb(p, q, m, t, narb),
                  "dust_density": nsc.dust_density_arb(p, q, m, t, s, narb),
                  "temperature": nsc.temperature_arb(p, q, m, t, T, narb),
                  "dust_temperature": nsc.dust_temperature_arb(p, q, m, t, s, T, narb),
                  "photoionization": nsc.photoionization_arb(p, q, m, kw["n_part"], kw["value"], t, narb)}
    finally:
        nsc.d = None
    for name in FIELDS:
        assert np.array_equal(single[name], got[name], equal_nan=True), name


@pytest.mark.parametrize("case", CASES)
def test_grid_form_matches_reference_on_the_exact_ball(case):
    import sph_code_amd.compat as nsc
    g, a, kw = case_inputs(case)
    q = a["arb_points"]
    o = arb_oracle.fields(arb_points=q, row_start=a["exact_row_start"], members=a["exact_members"], **kw)
    ball = nsc.neighbors_arb(kw["points"], q, kw["sizes"])
    assert len(ball) == q.shape[0] and ball.radius == float(a["radius"])
    got = gpu_fields(nsc, kw, q, ball)
    check_against(got, {n: a["exact_" + n] for n in FIELDS}, o, "%s grid form" % case)
    want = np.diff(a["exact_row_start"]).astype(np.int64)
    assert np.array_equal(got["count"], want)
    assert np.array_equal(ball.counts, want) and len(ball[3]) == want[3]
    assert got["candidates"] > 0
    # gate only (no counts asked for): the same fields, bit for bit
    lean = gpu_fields(nsc, kw, q, ball, with_stats=False)
    for name in FIELDS:
        assert np.array_equal(lean[name], got[name], equal_nan=True), name
    # the points beyond R from the box, alone: nothing is evaluated
    far = np.ascontiguousarray(q[-int(a["n_far"]):])
    gf = gpu_fields(nsc, kw, far, nsc.neighbors_arb(kw["points"], far, kw["sizes"]))
    assert gf["candidates"] == 0 and (gf["count"] == 0).all()
    for name in FIELDS:
        assert (gf[name] == 0.0).all(), name


@pytest.mark.parametrize("case", CASES)
def test_deterministic_and_independent_of_point_order(case):
    import sph_code_amd.compat as nsc
    g, a, kw = case_inputs(case)
    q = a["arb_points"]
    ball = nsc.neighbors_arb(kw["points"], q, kw["sizes"])
    one, two = gpu_fields(nsc, kw, q, ball), gpu_fields(nsc, kw, q, ball)
    perm = np.random.RandomState(7).permutation(q.shape[0])
    qp = np.ascontiguousarray(q[perm])
    three = gpu_fields(nsc, kw, qp, nsc.neighbors_arb(kw["points"], qp, kw["sizes"]))
    for name in FIELDS + ("count",):
        assert np.array_equal(one[name], two[name], equal_nan=True), name
        back = np.empty_like(three[name])
        back[perm] = three[name]
        assert np.array_equal(one[name], back, equal_nan=True), name
    rows = rows_of(a, "ref")
    l1, l2 = gpu_fields(nsc, kw, q, rows), gpu_fields(nsc, kw, q, rows)
    for name in FIELDS:
        assert np.array_equal(l1[name], l2[name], equal_nan=True), name


def test_larger_polytrope_slice_and_random_points():
    """A polytrope with its own kNN sizes and a tenth of it dust: a slice through the centre plus random points, against
    arb_oracle on the brute-force eps = 0 ball.  N = 100 000 particles, an 80 x 80 slice and 3 600 random points: 10^9
    brute-force distances and ~10^8 ball members on the host, about half a minute of the yardstick."""
    import sph_code_amd.compat as nsc
    from sph_code_amd import ics
    s = ics.polytrope_sphere(100000)
    rs = np.random.RandomState(99)
    n = s["points"].shape[0]
    ptype = np.zeros(n)
    ptype[rs.permutation(n)[:n // 10]] = 2.0                     # some dust, so that every field is exercised
    sizes = nsc.neighbors(s["points"], np.inf, 40)[4]
    kw = dict(points=s["points"], mass=s["mass"], particle_type=ptype, sizes=sizes, T=s["T"],
              n_part=10.0 ** rs.uniform(50.0, 54.0, n), value=10.0 ** rs.uniform(-12.0, -8.0, n),
              d=ics.loop_d(s, 40), m_0=nsc.m_0)
    lo, hi = s["points"].min(axis=0), s["points"].max(axis=0)
    q = np.concatenate([ics.slice_points(0.5 * (lo + hi), 2, (hi - lo)[:2] * 0.5, (80, 80)).reshape(-1, 3),
                        lo + rs.rand(3600, 3) * (hi - lo)])
    q = np.ascontiguousarray(q)
    R = float(np.max(sizes))
    o = oracle_chunked(kw, q, R)
    got = gpu_fields(nsc, kw, q, nsc.neighbors_arb(kw["points"], q, sizes))
    assert np.array_equal(got["count"], o["count"])
    check_against(got, o, o, "polytrope grid form")
    assert (o["density"] > 0).sum() > 1000 and (o["dust_density"] > 0).sum() > 100
    # the cost follows the supports, not R: every point lies inside the particles' box, so a ball 100 times wider
    # changes no culling decision - the same pair evaluations, the same sums, and every particle in every ball
    wide = gpu_fields(nsc, kw, q, nsc.ArbBall(kw["points"], q, 100.0 * R))
    assert wide["candidates"] == got["candidates"]
    assert (wide["count"] == n).all()
    assert 0 < got["candidates"] < q.shape[0] * n


def _sim_state(n=6000):
    from sph_code_amd import ics
    return ics.dusty_sphere(n, dust_frac=0.1)


def test_simulation_sample_matches_compat_and_leaves_the_loop_alone():
    import sph_code_amd.compat as nsc
    from sph_code_amd import ics
    from sph_code_amd.sim import Simulation
    s = _sim_state()
    n = s["points"].shape[0]
    d = ics.loop_d(s, 40)
    rs = np.random.RandomState(5)
    n_part, value = 10.0 ** rs.uniform(50.0, 54.0, n), 10.0 ** rs.uniform(-12.0, -8.0, n)
    # (the loop forms - the reference's own time loop - keep T positive; under hydro_update's sums T < 0 from the second
    #  step on, DESIGN 6.5, where temperature_arb's mask depends on the whole ball: sphx_arb_pair.h, clip)
    sim, twin = Simulation(s, n_neigh=40, forms="loop", d=d), Simulation(s, n_neigh=40, forms="loop", d=d)
    q0 = ics.slice_points((0.0, 0.0, 0.0), 2, 1.0e17, (8, 8))
    with pytest.raises(RuntimeError, match="-4"):                 # SPHX_E_STATE: sizes do not exist before the first step
        sim.sample(q0, d)
    sim.step(2)
    twin.step(2)
    st = sim.download()
    assert (st["T"] > 0).all()
    lo, hi = st["points"].min(axis=0), st["points"].max(axis=0)
    q = ics.slice_points(0.5 * (lo + hi), 2, (hi - lo)[:2], (48, 40))
    got = sim.sample(q, d, fields=FIELDS, n_part=n_part, value=value, with_stats=True)
    assert got["density"].shape == (48, 40) and got["count"].shape == (48, 40)
    kw = dict(points=st["points"], mass=s["mass"], particle_type=s["particle_type"], sizes=st["sizes"], T=st["T"],
              n_part=n_part, value=value, d=d, m_0=nsc.m_0)
    qf = np.ascontiguousarray(q.reshape(-1, 3))
    o = oracle_chunked(kw, qf, float(np.max(st["sizes"])))
    ref = gpu_fields(nsc, kw, qf, nsc.neighbors_arb(st["points"], qf, st["sizes"]))
    assert np.array_equal(got["count"].ravel(), ref["count"])
    assert (ref["density"] > 0).sum() > 100
    for name in FIELDS:
        # both evaluations lie within the bound of the yardstick: the particle order differs on the device
        arb_oracle.assert_within(name, ref[name], o[name], o[name + "_bound"], what="compat vs oracle")
        arb_oracle.assert_within(name, got[name].ravel(), o[name], o[name + "_bound"], what="sample vs oracle")
    # a third step after sampling: the bits of a twin that never sampled
    sim.step(1)
    twin.step(1)
    a, b = sim.download(), twin.download()
    for key in ("points", "velocities", "total_accel", "E_internal", "T", "sizes", "densities", "num_densities",
                "visc_heat", "pressure"):
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    assert a["dt"] == b["dt"]


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 4097])
def test_odd_point_counts(m):
    import sph_code_amd.compat as nsc
    g, a, kw = case_inputs("sphere_dust_n2048_k40")
    rs = np.random.RandomState(100 + m)
    lo, hi = kw["points"].min(axis=0), kw["points"].max(axis=0)
    q = np.ascontiguousarray(lo + rs.rand(m, 3) * (hi - lo))
    got = gpu_fields(nsc, kw, q, nsc.neighbors_arb(kw["points"], q, kw["sizes"]))
    o = oracle_chunked(kw, q, float(a["radius"])) if m else None
    for name in FIELDS:
        assert got[name].shape == (m,)
    if m:
        assert np.array_equal(got["count"], o["count"])
        check_against(got, o, o, "M = %d" % m)
        rows_rs, rows_mem = arb_oracle.brute_ball(kw["points"], q, float(a["radius"]))
        rows = [rows_mem[rows_rs[j]:rows_rs[j + 1]] for j in range(m)]
        check_against(gpu_fields(nsc, kw, q, rows), o, o, "M = %d list form" % m)
    else:
        assert gpu_fields(nsc, kw, q, [])["candidates"] == 0


def test_degenerate_inputs():
    import sph_code_amd.compat as nsc
    g, a, kw = case_inputs("sphere_dust_n2048_k40")
    q = np.ascontiguousarray(a["arb_points"][:200])
    R = float(a["radius"])
    # N = 1: every gate is off
    one = {k: (v[:1] if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    q1 = np.ascontiguousarray(np.concatenate([one["points"], one["points"] + 0.1 * one["sizes"][0]]))
    g1 = gpu_fields(nsc, one, q1, nsc.neighbors_arb(one["points"], q1, one["sizes"]))
    assert list(g1["count"]) == [1, 1]
    for name in FIELDS:
        assert (g1[name] == 0.0).all(), name
    # all-gas and all-dust particle sets
    for t in (0.0, 2.0):
        k2 = dict(kw, particle_type=np.full_like(kw["particle_type"], t))
        o = oracle_chunked(k2, q, R)
        got = gpu_fields(nsc, k2, q, nsc.neighbors_arb(k2["points"], q, k2["sizes"]))
        check_against(got, o, o, "all type %g" % t)
        assert np.array_equal(got["count"], o["count"])
        assert (got["density" if t == 0.0 else "dust_density"] > 0).any()
        assert (got["dust_density" if t == 0.0 else "density"] == 0).all()
    # sizes, T, n_part, value all missing: only density is produced (the ball radius is then given)
    bare = dict(points=kw["points"], mass=kw["mass"], particle_type=kw["particle_type"], d=kw["d"])
    ball = nsc.ArbBall(kw["points"], q, R)
    got = gpu_fields(nsc, bare, q, ball, fields=("density",))
    o = oracle_chunked(kw, q, R)
    arb_oracle.assert_within("density", got["density"], o["density"], o["density_bound"], what="density alone")
    with pytest.raises(ValueError):
        gpu_fields(nsc, bare, q, ball, fields=("temperature",))
    # NaN / inf coordinates: count 0 and zeros; the other points are not affected
    qb = q.copy()
    qb[3, 0] = np.nan
    qb[7, 2] = np.inf
    gb = gpu_fields(nsc, kw, qb, nsc.neighbors_arb(kw["points"], qb, kw["sizes"]))
    full = gpu_fields(nsc, kw, q, nsc.neighbors_arb(kw["points"], q, kw["sizes"]))
    keep = np.ones(len(q), bool)
    keep[[3, 7]] = False
    for name in FIELDS + ("count",):
        assert (gb[name][~keep] == 0).all(), name
        assert np.array_equal(gb[name][keep], full[name][keep], equal_nan=True), name
    # argument errors
    c = nsc.context()
    dp, ip = nsc.dp, nsc.ip
    out = np.zeros(4)
    cand = np.zeros(1, np.int64)
    args = (dp(kw["points"]), dp(kw["mass"]), dp(kw["particle_type"]), None, None, None, None, kw["d"])
    tail = (dp(out), None, None, None, None, None, ip(cand), 0)
    assert c.lib.sphx_arb_fields(c.h, 0, *args, 4, dp(q), R, *tail) == -1
    assert c.lib.sphx_arb_fields(c.h, 10, *args, -1, dp(q), R, *tail) == -1
    assert c.lib.sphx_arb_fields(c.h, 10, *args, 4, dp(q), 0.0, *tail) == -1          # radius <= 0 without sizes
    assert c.lib.sphx_arb_fields(c.h, 10, *args, 4, None, R, *tail) == -1             # NULL required pointers
    for hole in range(3):
        holed = list(args)
        holed[hole] = None
        assert c.lib.sphx_arb_fields(c.h, 10, *holed, 4, dp(q), R, *tail) == -1, hole
    assert c.lib.sphx_arb_fields(c.h, 10, *args, 0, None, R, *tail) == 0              # m = 0 is fine
    bad_rs = np.array([0, 2, 1, 3, 3], np.int64)
    mem = np.zeros(3, np.int64)
    assert c.lib.sphx_arb_fields_list(c.h, 10, *args, 4, dp(q), ip(bad_rs), ip(mem), dp(out), None, None, None, None,
                                      None, ip(cand)) == -1
    # ids outside 0 .. n-1 are skipped
    rows = [[-1, 0, 1, 5000], [0, 1]]
    q2 = np.ascontiguousarray(kw["points"][:2])
    gl = gpu_fields(nsc, kw, q2, rows)
    o2 = arb_oracle.fields(arb_points=q2, row_start=[0, 2, 4], members=[0, 1, 0, 1], **kw)
    assert list(gl["count"]) == [4, 2]
    check_against(gl, o2, o2, "ids skipped")


def test_calls_on_one_handle_reuse_the_ball():
    """The reference's call sequence - one neighbors_arb, then the five functions on its result - builds the cell list
    and sorts the query points once: a call that names a held ball reads neither points nor arb_points."""
    import sph_code_amd.compat as nsc
    g, a, kw = case_inputs("sphere_dust_n2048_k40")
    q = a["arb_points"]
    o = arb_oracle.fields(arb_points=q, row_start=a["exact_row_start"], members=a["exact_members"], **kw)
    p, m, t, s, T = kw["points"], kw["mass"], kw["particle_type"], kw["sizes"], kw["T"]
    nsc.d = kw["d"]
    try:
        narb = nsc.neighbors_arb(p, q, s)
        got = {"density": nsc.density_arb(p, q, m, t, narb)}
        nsc.neighbors(p, np.inf, 8)                       # another entry point in between: its scratch is not the ball's
        got["dust_density"] = nsc.dust_density_arb(p, q, m, t, s, narb)
        got["temperature"] = nsc.temperature_arb(p, q, m, t, T, narb)
        got["dust_temperature"] = nsc.dust_temperature_arb(p, q, m, t, s, T, narb)
        got["photoionization"] = nsc.photoionization_arb(p, q, m, kw["n_part"], kw["value"], t, narb)
        assert np.array_equal(narb.counts, np.diff(a["exact_row_start"]))
        assert len(narb[5]) == int(np.diff(a["exact_row_start"])[5])
        with pytest.raises(ValueError):                   # a handle is for its own positions and points
            nsc.density_arb(p + 1.0, q, m, t, narb)
        with pytest.raises(ValueError):
            nsc.density_arb(p, q[::-1].copy(), m, t, narb)
    finally:
        nsc.d = None
    check_against(got, {n: a["exact_" + n] for n in FIELDS}, o, "five calls on one handle")
    # at the C boundary: the second call with the same ball_id is handed zeros for points and arb_points and must not
    # notice; with ball_id = 0 it does
    c = nsc.context()
    dp, ip = nsc.dp, nsc.ip
    n, M = p.shape[0], q.shape[0]
    R = float(a["radius"])
    cand = np.zeros(1, np.int64)

    def call(points, arb, ball_id):
        out = np.zeros(M)
        assert c.lib.sphx_arb_fields(c.h, n, dp(points), dp(m), dp(t), dp(s), dp(T), None, None, kw["d"], M, dp(arb), R,
                                     dp(out), None, None, None, None, None, ip(cand), ball_id) == 0
        return out

    first = call(p, q, 123456789)
    again = call(np.zeros_like(p), np.zeros_like(q), 123456789)
    assert np.array_equal(first, again) and (first > 0).sum() > 50
    fresh = call(np.zeros_like(p), np.zeros_like(q), 0)
    assert not np.array_equal(first, fresh)
    t_ms = nsc.arb_last_timing()
    assert set(t_ms) == {"upload", "build", "kernels", "download"} and all(v >= 0.0 for v in t_ms.values())


@pytest.mark.parametrize("incremental", [False, True])
def test_sample_under_hydro_update_forms(incremental):
    """The default step (hydro_update's sums) leaves negative temperatures behind from the second step on.
    The grid form counts a particle in temperature only inside its own support and with Wg T > 0 - that is, with
    T > 0: the reference's formula on max(T, 0), whose mask Wg max(T, 0) > 0 says the same.  The other fields are not
    affected; and the loop is left alone in this mode too, with and without the incremental search."""
    import sph_code_amd.compat as nsc
    from sph_code_amd import ics
    from sph_code_amd.sim import Simulation
    s = _sim_state()
    d = ics.loop_d(s, 40)
    sim = Simulation(s, n_neigh=40, incremental=incremental)
    twin = Simulation(s, n_neigh=40, incremental=incremental)
    sim.step(2)
    twin.step(2)
    st = sim.download()
    assert (st["T"] < 0).sum() > 100
    lo, hi = st["points"].min(axis=0), st["points"].max(axis=0)
    q = ics.slice_points(0.5 * (lo + hi), 1, (hi - lo)[[0, 2]] * 0.5, (24, 24))
    got = sim.sample(q, d, fields=("density", "dust_density", "temperature"))
    assert (got["density"] > 0).sum() > 100 and (got["temperature"] >= 0.0).all()
    kw = dict(points=st["points"], mass=s["mass"], particle_type=s["particle_type"], sizes=st["sizes"],
              T=np.maximum(st["T"], 0.0), n_part=None, value=None, d=d, m_0=nsc.m_0)
    o = oracle_chunked(kw, np.ascontiguousarray(q.reshape(-1, 3)), float(np.max(st["sizes"])))
    for name in ("density", "dust_density", "temperature"):
        arb_oracle.assert_within(name, got[name].ravel(), o[name], o[name + "_bound"], what="hydro_update forms")
    sim.step(2)
    twin.step(2)
    a, b = sim.download(), twin.download()
    for key in ("points", "velocities", "total_accel", "E_internal", "T", "sizes", "densities", "num_densities",
                "visc_heat", "pressure"):
        assert np.array_equal(a[key], b[key], equal_nan=True), key
