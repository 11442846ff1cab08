"""GPU tests (-m gpu): the search, the sums, the fused step and the samplers on the transformed clouds of tests/frames.py -
off-centre by up to 2^27 cloud sizes, rescaled, flattened to sheets, planes, needles and lines, split into far-apart
clumps.  tests/test_frames_cpu.py shows the cases sound.  Two references: the CPU oracle with the bounds of
tests/oracle_bounds.py (no new tolerance), and, for shifts and scalings by powers of two, the same call on the untransformed
cloud, bit for bit (coordinate differences of the snapped clouds are exact, so every pair term sees the same operands)."""
import numpy as np
import pytest

import arb_oracle
import frames
import oracle_bounds as ob
from test_frames_cpu import STEP_CASES, step_fixed_dt
from test_odd_shapes_cpu import hydro_modes, oracle_step

pytestmark = pytest.mark.gpu

SLOW = ("two_clumps", "clumps_shifted")


def _cases(cases, frame_at=0):
    return [pytest.param(c, id=frames.case_id(c), marks=[pytest.mark.timeout(180)] if c[frame_at] in SLOW else [])
            for c in cases]


@pytest.fixture(scope="module")
def nsc():
    import sph_code_amd.compat as nsc_mod
    nsc_mod.context()
    return nsc_mod


LOOP_NAMES = ("density", "dust_density", "num_dens", "del_pressure", "av accel", "av heat", "crossing_time", "drag onto",
              "drag reaction")


def _gpu_outputs(nsc, s, d, K):
    """Everything the array API computes on one cloud -> dict (search, hydro_update per mode, loop forms)."""
    p, v = s["points"], s["velocities"]
    idx, _, dist, nontriv, h = nsc.neighbors(p, np.inf, K)
    m, pt, mu, gam = s["mass"], s["particle_type"], s["mu_array"], s["gamma_array"]
    out = dict(idx=np.array(idx), dist=np.array(dist), nontriv=nontriv, h=h)
    args = (idx, p, m, h, s["f_un"], pt, s["T"], mu, gam, v)
    for mode in hydro_modes(K):
        out[mode] = nsc.hydro_update(*args, clip_grad=mode[1], visc_mode=mode[0])
    d_before = nsc.d
    nsc.d = d
    try:
        rho = nsc.density(p, m, pt, idx)
        acc, heat = nsc.artificial_viscosity(idx, p, pt, h, m, rho, v, s["T"], gam, mu)
        onto, react = nsc.net_impulse(p, m, h, v, pt, idx, s["f_un"])
        out["loop"] = dict(zip(LOOP_NAMES, (rho, nsc.dust_density(p, m, idx, pt, h), nsc.num_dens(m, p, mu, idx),
                                            nsc.del_pressure(p, m, pt, idx, s["E_internal"], gam), acc, heat,
                                            nsc.crossing_time(idx, v, h, pt), onto, react)))
    finally:
        nsc.d = d_before
    return out


_base_outputs = {}


def _base(nsc, meta, workload, n, K):
    key = (workload, n, K)
    if key not in _base_outputs:
        _base_outputs[key] = _gpu_outputs(nsc, meta["base"], meta["base_d"], K)
    return _base_outputs[key]


@pytest.mark.parametrize("case", _cases(frames.CASES))
def test_array_api_vs_oracle_on_transformed_clouds(nsc, case):
    """test_array_api_vs_oracle_at_odd_shapes on every frame, unclamped: distance rows to rtol 2e-15 on every row, index
    sets on the rows without a tie at the K-th distance, then hydro_update in its four modes and the loop forms with
    net_impulse, every row within the bounds of tests/oracle_bounds.py on the GPU's own idx, h."""
    from oracle import sph_oracle as orc
    frame, workload, n, K = case
    s, d, meta = frames.frame_case(*case)
    p, v = s["points"], s["velocities"]
    idx, _, dist, nontriv, h = nsc.neighbors(p, np.inf, K)
    oi, _, od, ont, oh = orc.neighbors(p, np.inf, K, eps=0.0)
    np.testing.assert_allclose(dist, od, rtol=2e-15, atol=0)
    untied = ~frames.tied_rows(p, K)
    assert (np.sort(idx, axis=1)[untied] == np.sort(oi, axis=1)[untied]).all() and np.array_equal(nontriv, ont)
    assert (nontriv == K).all() and not (idx == n).any()
    m, pt, mu, gam = s["mass"], s["particle_type"], s["mu_array"], s["gamma_array"]
    args = (idx, p, m, h, s["f_un"], pt, s["T"], mu, gam, v)
    for visc_mode, clip_grad in hydro_modes(K):
        out = nsc.hydro_update(*args, clip_grad=clip_grad, visc_mode=visc_mode)
        ref, scales = ob.hydro_reference(args, clip_grad=clip_grad, visc_mode=visc_mode)
        ob.compare_hydro(out, ref, scales, "%s %s clip=%d" % (frames.case_id(case), visc_mode, clip_grad))
    d_before = nsc.d
    nsc.d = d
    try:
        rho = nsc.density(p, m, pt, idx)
        ref = ob.loop_reference(p, v, m, pt, h, idx, d, s["E_internal"], s["T"], gam, mu, rho, f_un=s["f_un"], workers=1)
        drag = ob.compare_loop(nsc, ref, p, v, m, pt, h, idx, d, s["E_internal"], s["T"], gam, mu, rho,
                               frames.case_id(case), f_un=s["f_un"])
    finally:
        nsc.d = d_before
    if workload == "two_phase":
        assert np.abs(drag[0]).max() > 0 and np.abs(drag[1]).max() > 0


def _same(got, base, power, scale, what):
    want = np.asarray(base) * scale ** power
    assert np.array_equal(np.asarray(got), want, equal_nan=True), \
        "%s: %d elements differ from the untransformed call" % (what, (np.asarray(got) != want).sum())


@pytest.mark.parametrize("case", _cases([c for c in frames.CASES if c[0] in frames.SHIFTS + frames.SCALES]))
def test_array_api_is_frame_invariant_bit_for_bit(nsc, case):
    """The same calls on the snapped, untransformed cloud: dist, h (x the scale), nontriv and the sorted idx of untied rows
    identical, every output of hydro_update and of the loop forms identical for shifts and exactly rescaled by the known
    power of two for scalings (frames.HYDRO_POWERS, frames.LOOP_POWERS)."""
    frame, workload, n, K = case
    s, d, meta = frames.frame_case(*case)
    sc = meta["scale"]
    got, base = _gpu_outputs(nsc, s, d, K), _base(nsc, meta, workload, n, K)
    what = frames.case_id(case)
    _same(got["dist"], base["dist"], 1, sc, what + " dist")
    _same(got["h"], base["h"], 1, sc, what + " h")
    assert np.array_equal(got["nontriv"], base["nontriv"])
    untied = ~frames.tied_rows(meta["base"]["points"], K)
    assert (np.sort(got["idx"], axis=1)[untied] == np.sort(base["idx"], axis=1)[untied]).all()
    for mode in hydro_modes(K):
        for i, name in enumerate(ob.HYDRO_NAMES):
            _same(got[mode][i], base[mode][i], frames.HYDRO_POWERS[i], sc, "%s %s %s" % (what, mode, name))
    for name in LOOP_NAMES:
        _same(got["loop"][name], base["loop"][name], frames.LOOP_POWERS[name], sc, "%s loop %s" % (what, name))


def _first_grid(points, K):
    """The grid of the first search on a fresh context (the module context keeps state between calls)."""
    from sph_code_amd import _lib
    from sph_code_amd._lib import dp, ip
    p = np.ascontiguousarray(points)
    n = len(p)
    c = _lib.Context()
    idx, dd, nt, h = np.empty((n, K), np.int64), np.empty((n, K)), np.empty(n, np.int64), np.empty(n)
    c.check(c.lib.sphx_neighbors(c.h, n, K, dp(p), 0.0, 0.0, ip(idx), dp(dd), ip(nt), dp(h)))
    st = c.stats()
    c.close()
    return st, h


def _check_grid(points, K, what):
    n = len(points)
    cell, nx, ny, nz = frames.grid_rule(points, n, K)
    st, _ = _first_grid(points, K)
    print("%s: cell_size %.17g (rule %.17g), cells %d (rule %d x %d x %d = %d)"
          % (what, st["cell_size"], cell, st["cells"], nx, ny, nz, nx * ny * nz))
    assert abs(st["cell_size"] - cell) <= 1e-9 * cell, (what, st["cell_size"], cell)
    # one layer per axis; an axis of one cell by the rule (a plane, a line, a sheet) has no layer to give: its extent is
    # far below a cell, no floor() sits near an integer there, and its 1/1 would make the bound the whole count
    layers = sum(1.0 / c for c in (nx, ny, nz) if c > 1)
    assert abs(st["cells"] - nx * ny * nz) <= layers * nx * ny * nz, (what, st["cells"], (nx, ny, nz))


@pytest.mark.parametrize("case", _cases([c for c in frames.CASES if c[0] not in frames.SCALES]))
def test_first_grid_follows_the_sizing_rule(case):
    """stats() after the first search of a fresh context against frames.grid_rule: cell_size to rtol 1e-9, the
    cell count within one layer per axis that has more than one cell (a floor() may sit on an integer; the stats do not
    expose nx, ny, nz)."""
    s, _, _ = frames.frame_case(*case)
    _check_grid(s["points"], case[3], frames.case_id(case))


def test_first_grid_follows_the_sizing_rule_on_a_heavy_tailed_cloud_far_from_the_origin():
    """The core + halo cloud (46 000 particles, the 3 sigma clip active by design) 2^27 core sizes from the origin.  Its sigma
    (3e20 m) is set by the halo, so T / sigma is only 1e5 and the raw-moment variance var = sq/cnt - mean^2 was still good to
    1e-7 here; what missed the gate before the moments and the box were taken about a pivot was the ulp of the absolute
    box corners (2^27 R0: cell_size off by 3.7e-9).  By reading, not measured: sigma itself is lost to raw moments only at
    T / sigma >= 1e7, which no cloud of this suite reaches."""
    p, off = frames.heavy_tailed_cloud()
    _check_grid(p + off, 40, "heavy-tailed shift_27")


@pytest.mark.parametrize("case", _cases(STEP_CASES, frame_at=1))
def test_fused_step_vs_oracle_on_transformed_clouds(case):
    """Simulation.step for three steps against the oracle's step of the same mode with the gates of
    test_fused_step_vs_oracle_at_odd_shapes; x to 1e-12 of the cloud's OWN size R0 (not max|x|, which the offset or the
    second clump's distance would inflate).  The plane and the needle run under a fixed Courant dt
    (test_frames_cpu.STEP_FIXED_DT)."""
    from sph_code_amd.sim import Simulation
    forms, frame, workload, n, K = case
    s0, d, meta = frames.frame_case(*case[1:])
    fixed_dt = step_fixed_dt(case, s0)
    kw = dict(forms="loop", d=d, with_drag=(workload == "two_phase")) if forms == "loop" else \
        dict(visc_mode="pairwise" if forms == "pairwise" else "ref_axis0")
    sim = Simulation(s0, n_neigh=K, **kw)
    ref = dict(s0)
    ocase = (forms, workload, n, K)
    for it in range(3):
        sim.step(1, fixed_dt=fixed_dt)
        ref = oracle_step(ocase, ref, d, it == 0, fixed_dt)
        got = sim.download()
        assert got["dt"] == pytest.approx(ref["dt"], rel=1e-12), "dt at step %d" % it
    for key in ("points", "velocities", "sizes", "densities"):
        assert np.isfinite(ref[key]).all() and np.isfinite(got[key]).all(), key
    ex = np.max(np.abs(got["points"] - ref["points"])) / meta["R0"]
    ev = np.max(np.abs(got["velocities"] - ref["velocities"])) / np.max(np.abs(ref["velocities"]))
    print("%s: x err %.3g of R0, v err %.3g of max|v|" % (frames.case_id(case), ex, ev))
    assert ex <= 1e-12 and ev <= 1e-10
    np.testing.assert_allclose(got["sizes"], ref["sizes"], rtol=1e-9)
    np.testing.assert_allclose(got["densities"], ref["densities"], rtol=1e-9)
    assert np.any(got["total_accel"] != 0.0)


@pytest.mark.parametrize("case", _cases(STEP_CASES, frame_at=1))
def test_hinted_search_is_exact_on_transformed_clouds(case, monkeypatch):
    """The step loop's hinted search (grouped kernel: tile-relative fp32 coordinates, order certified or handed on) under
    flat tiles, tiles 2^12 cloud sizes from the origin and crowded cells: the radii of every step equal the exact
    K-th-neighbour distance (cKDTree, eps = 0, on the downloaded positions) bit for bit, no short row, and the trajectory
    without the grouped kernel (SPHX_KNN_GROUP=0) is the same bits.  fallback_queries is printed, not asserted: how many
    queries a flat or crowded tile can certify has not been measured."""
    from oracle import sph_oracle as orc
    from sph_code_amd.sim import Simulation
    forms, frame, workload, n, K = case
    s0, d, meta = frames.frame_case(*case[1:])
    kw = dict(forms="loop", d=d, with_drag=(workload == "two_phase")) if forms == "loop" else \
        dict(visc_mode="pairwise" if forms == "pairwise" else "ref_axis0")
    res = {}
    for group in ("1", "0"):
        monkeypatch.setenv("SPHX_KNN_GROUP", group)
        sim = Simulation(s0, n_neigh=K, **kw)
        pts = s0["points"]
        for it in range(3):
            _, _, _, _, h_ref = orc.neighbors(pts, np.inf, K, eps=0.0)
            sim.step(1, fixed_dt=1e-30)
            got = sim.download()
            assert np.array_equal(got["sizes"], h_ref), (group, it, np.abs(got["sizes"] - h_ref).max())
            pts = got["points"]
        st = sim.stats()
        assert st["short_rows"] == 0
        print("%s SPHX_KNN_GROUP=%s: fallback_queries %d of %d" % (frames.case_id(case), group, st["fallback_queries"], 3 * n))
        res[group] = got
    for key in ("points", "velocities", "E_internal", "T", "sizes", "densities", "total_accel"):
        assert np.array_equal(res["1"][key], res["0"][key], equal_nan=True), key


ARB_N, ARB_K = 4097, 40


def _arb_queries(p, sizes, rs, flat):
    """1000 points: half on particles, half uniform in the bounding box (a planar cloud: half of those off the plane)."""
    lo, hi = p.min(axis=0), p.max(axis=0)
    u = lo + rs.rand(500, 3) * (hi - lo)
    if flat:
        u[:250, 2] += (rs.rand(250) - 0.5) * np.median(sizes)
    return np.concatenate([p[rs.choice(len(p), 500, replace=False)], u])


@pytest.mark.parametrize("frame", [pytest.param(f, marks=[pytest.mark.timeout(180)] if f in SLOW else [])
                                   for f in ("shift_27", "scale_down", "plane", "two_clumps")])
def test_samplers_on_transformed_clouds(nsc, frame):
    """compat.arb_fields (grid form) and Simulation.sample against tests/arb_oracle.py on the brute-force eps = 0 ball, to
    that module's bounds; the shifted cloud also against the unshifted call, both samplers, bit for bit.  (Simulation
    applies the reference's position clamp: the contexts of that part carry a clamp beyond the offset.)"""
    from sph_code_amd import _lib
    from sph_code_amd.sim import Simulation
    from test_gpu_arb import FIELDS, check_against, gpu_fields, oracle_chunked
    s, d, meta = frames.frame_case(frame, "two_phase", ARB_N, ARB_K)
    sc, off = meta["scale"], meta["offset"]
    rs = np.random.RandomState(11)
    n_part, value = 10.0 ** rs.uniform(50.0, 54.0, ARB_N), 10.0 ** rs.uniform(-12.0, -8.0, ARB_N)

    def inputs(state, dd):
        sizes = nsc.neighbors(state["points"], np.inf, ARB_K)[4]
        return dict(points=state["points"], mass=state["mass"], particle_type=state["particle_type"], sizes=sizes,
                    T=state["T"], n_part=n_part, value=value, d=dd, m_0=nsc.m_0)
    kw = inputs(s, d)
    if meta["kind"] in ("shift", "scale"):                       # queries on the lattice of the base cloud, then transformed
        kb = inputs(meta["base"], meta["base_d"])
        qb = np.round(_arb_queries(kb["points"], kb["sizes"], rs, False) / meta["q"]) * meta["q"]
        q = np.ascontiguousarray(qb * sc + off)
    else:
        q = np.ascontiguousarray(_arb_queries(kw["points"], kw["sizes"], rs, frame == "plane"))
    o = oracle_chunked(kw, q, float(np.max(kw["sizes"])))
    got = gpu_fields(nsc, kw, q, nsc.neighbors_arb(kw["points"], q, kw["sizes"]))
    assert np.array_equal(got["count"], o["count"])
    check_against(got, o, o, "%s grid form" % frame)
    assert (o["density"] > 0).sum() > 400 and (o["dust_density"] > 0).sum() > 50
    if meta["kind"] == "shift":
        gb = gpu_fields(nsc, kb, np.ascontiguousarray(qb), nsc.neighbors_arb(kb["points"], np.ascontiguousarray(qb), kb["sizes"]))
        assert np.array_equal(got["count"], gb["count"])
        for name in FIELDS:
            assert np.array_equal(got[name], gb[name], equal_nan=True), name
    clamp = max(1e11 * 149597870700.0, 4.0 * np.abs(s["points"]).max())

    def sampled(state, dd, queries):
        ctx = _lib.Context()
        try:
            ctx.set_constants(k_B=nsc.k, amu=nsc.amu, m_h=nsc.m_h, m_0=nsc.m_0, dt_0=nsc.dt_0, pos_clamp=clamp)
            sim = Simulation(state, n_neigh=ARB_K, forms="loop", d=dd, ctx=ctx)
            sim.step(1, fixed_dt=1e-30)
            return sim.download(), sim.sample(queries, dd, fields=FIELDS, n_part=n_part, value=value, with_stats=True)
        finally:
            ctx.close()
    st, smp = sampled(s, d, q)
    kws = dict(kw, points=st["points"], sizes=st["sizes"], T=st["T"])
    os_ = oracle_chunked(kws, q, float(np.max(st["sizes"])))
    assert np.array_equal(smp["count"], os_["count"])
    check_against(smp, os_, os_, "%s Simulation.sample" % frame)
    if meta["kind"] == "shift":
        stb, sb = sampled(meta["base"], meta["base_d"], np.ascontiguousarray(qb))
        assert np.array_equal(st["points"] - off, stb["points"]) and np.array_equal(st["sizes"], stb["sizes"])
        differ = [name for name in ("count",) + tuple(FIELDS) if not np.array_equal(smp[name], sb[name], equal_nan=True)]
        assert not differ, "Simulation.sample differs from the unshifted call in %s" % differ
