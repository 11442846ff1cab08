"""GPU tests (-m gpu) of the projected maps (include/sphx.h sphx_project_maps, sphx_state_project).

Array call: compat.project_maps against the NumPy restatement tests/map_oracle.py on every case of tests/map_cases.py, no
pixel left out.  The two sides form every operation of a term alike; what may differ by an ulp is cbrt in a gas row's
radius, so the bounds are the project's, not equality:
    columns        |got - ref| <= 1e-12 sum|term| per pixel (the per-row bound of test_gpu_oracle_full_size.py)
    temperatures   2.1e-12 relative: two such sums of positive terms and a division
    count, skipped, pairs   equal - tests/test_map_cpu.py checks that no pair of any case lies within 8 ulp of a support's
                   edge, where an ulp of the radius would decide.
Resident: Simulation.project against compat.project_maps on download(), bit for bit, and twin Simulations."""
import itertools

import numpy as np
import pytest

import map_cases as mc
import map_oracle as mo
import phase_fixture as pf

pytestmark = pytest.mark.gpu
SMALL = pf.SHAPES[1]                     # n = 257, K = 40, S = 15
TWO_PHASE = pf.SHAPES[4]                 # n = 2049, K = 40, S = 32
FLOAT_FIELDS = mo.FIELDS[:4]


@pytest.fixture(scope="module")
def nsc():
    import sph_code_amd.compat as nsc_mod
    nsc_mod.context()
    assert nsc_mod.m_0 == mc.M_0 and nsc_mod.MAP_FIELDS == mo.FIELDS
    return nsc_mod


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float64:
        return bool(np.array_equal(a, b))
    return bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.uint64), b[~np.isnan(b)].view(np.uint64)))


def same_maps(a, b, keys=mo.FIELDS + ("skipped", "pairs")):
    return all(same_bits(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k] for k in keys)


def call(nsc, case, **kw):
    s = case["state"]
    args = dict(axes=case["axes"], center=case["center"], half_width=case["half_width"], npix=case["npix"], depth=case["depth"])
    args.update(kw)
    return nsc.project_maps(s["points"], s["mass"], s["particle_type"], s["sizes"], s["T"], s["d"], **args)


def assert_against_restatement(got, ref, what):
    nu_nv = ref["count"].shape
    for f in mo.FIELDS:
        assert got[f].shape == nu_nv, (what, f, got[f].shape)
    worst = {}
    for f in ("gas_column", "dust_column"):
        err, scale = np.abs(got[f] - ref[f]), ref[f + "_abs"]
        worst[f] = float(np.max(np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), 0.0)))
        print(what, f, "worst |got - ref| / sum|term| = %.3g" % worst[f])
        assert np.all(err <= 1e-12 * scale), (what, f, worst[f])
    for f in ("gas_temperature", "dust_temperature"):
        g, r = got[f], ref[f]
        assert np.array_equal(np.isnan(g), np.isnan(r)), (what, f, "NaN pixels differ")
        ok = ~np.isnan(r)
        err = np.abs(g[ok] - r[ok])
        rel = float(np.max(np.where(r[ok] != 0, err / np.where(r[ok] != 0, np.abs(r[ok]), 1.0), err), initial=0.0))
        print(what, f, "worst relative = %.3g" % rel)
        assert np.all(err <= 2.1e-12 * np.abs(r[ok])), (what, f, rel)
    assert np.array_equal(got["count"], ref["count"]) and got["count"].dtype == np.int64, (what, "count")
    assert ref["edge"] == 0 and ref["box_edge"] == 0, (what, "a pair on a support's edge: the counts may not be compared")
    assert got["skipped"] == ref["skipped"] and got["pairs"] == ref["pairs"], (what, got["skipped"], ref["skipped"], got["pairs"], ref["pairs"])


# ---------------------------------------------------------------------------------------------------------------------
# array call
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_array_call_against_the_restatement(nsc, name):
    ref = mc.reference(name)
    got = call(nsc, mc.CASES[name])
    assert_against_restatement(got, ref, name)
    if name == "beside":
        assert got["pairs"] == 0 and not any(np.any(got[f]) for f in mo.FIELDS)
    if name == "all-stars":
        assert got["pairs"] == 0 and got["skipped"] == 0 and not np.any(got["count"])
    if name == "between-centres":
        assert got["count"].sum() == 1 and got["pairs"] == 2          # the first disc lists no tile, the third one and adds nothing
    if name == "long-list":
        assert got["count"].max() == 3000
    if name == "gas-only-and-dust-only-pixels":
        gas_only = (got["gas_column"] > 0) & (got["dust_column"] == 0)
        dust_only = (got["dust_column"] > 0) & (got["gas_column"] == 0)
        assert gas_only.any() and dust_only.any()
        assert np.all(got["dust_temperature"][gas_only] == 0) and np.all(got["gas_temperature"][dust_only] == 0)
        assert np.all(got["gas_temperature"][gas_only] == 100.0)      # the row with T < 0 has dropped out of both sums
    if name == "zoom20":
        assert got["count"].min() > 100                               # every pixel lies under hundreds of footprints


def test_the_depth_slab_is_half_open(nsc):
    """A particle exactly at lo is in, one exactly at hi is out: the two slabs of map_cases differ by those two rows."""
    lo, hi = mc.CASES["slab-lo-at-a-particle"], mc.CASES["slab-hi-at-a-particle"]
    s = lo["state"]
    x = s["points"][:, 0]
    in_lo = (x >= lo["depth"][0]) & (x < lo["depth"][1])
    in_hi = (x >= hi["depth"][0]) & (x < hi["depth"][1])
    assert np.count_nonzero(x == lo["depth"][0]) == 1 and np.count_nonzero(x == hi["depth"][1]) == 1
    assert in_lo[x == lo["depth"][0]].all() and not in_hi[x == hi["depth"][1]].any()
    assert np.count_nonzero(in_lo) == np.count_nonzero(in_hi) + 1
    # the slab equals the projection of its rows alone, bit for bit
    for case, keep in ((lo, in_lo), (hi, in_hi)):
        sub = dict(case, state={k: (v[keep] if isinstance(v, np.ndarray) else v) for k, v in s.items()}, depth=None)
        assert same_maps(call(nsc, case), call(nsc, sub))


def test_null_outputs_keep_the_bits_of_the_others(nsc):
    case = mc.CASES["negative-T"]
    full = call(nsc, case)
    for r in (1, 2):
        for fields in itertools.combinations(mo.FIELDS, r):
            got = call(nsc, case, fields=fields)
            assert set(got) == set(fields) | {"skipped", "pairs"}, fields
            assert same_maps(got, full, fields + ("skipped", "pairs")), fields
    none = call(nsc, case, fields=())
    assert none == dict(skipped=full["skipped"], pairs=full["pairs"])


def test_repeated_calls_and_storage_order(nsc):
    """Two calls give the same bits; so does the same cloud given in another order with the ids' order kept - here: the
    case itself against a call in between on another image (the buffers are reused, the lists rebuilt)."""
    case = mc.CASES["sphere_dust_n2048_k40-33x65"]
    a = call(nsc, case)
    call(nsc, mc.CASES["long-list"])
    b = call(nsc, case)
    assert same_maps(a, b)
    t = nsc.map_last_timing()
    assert tuple(t) == nsc.MAP_STAGES and all(v >= 0 for v in t.values()) and t["tiles"] > 0


# ---------------------------------------------------------------------------------------------------------------------
# resident
# ---------------------------------------------------------------------------------------------------------------------
def make_sim(spec, steps=0, forms=None):
    from sph_code_amd.sim import Simulation
    f = pf.state(*spec)
    mode = dict(forms="loop", d=f["d"]) if forms == "loop" else {}
    sim = Simulation(pf.sim_state(f), n_neigh=f["neighbor"].shape[1], with_species=True, **mode)
    for _ in range(steps):
        sim.step(1, fixed_dt=f["fixed_dt"])
    return sim, f


def window_of(st):
    return 1.05 * float(np.max(np.abs(st["points"][:, 1:])))


def array_project(nsc, sim, f, d, hw, npix, **kw):
    st = sim.download()
    return nsc.project_maps(st["points"], f["mass"], sim._ptype, st["sizes"], st["T"], d, half_width=hw, npix=npix, **kw), st


@pytest.mark.parametrize("spec", [SMALL, TWO_PHASE], ids=["n257", "n2049"])
def test_resident_call_is_the_array_call_on_the_downloaded_state(nsc, spec):
    sim, f = make_sim(spec, forms="loop")
    hw = None
    for steps in (1, 2):                                              # after 1 and after 3 steps: the state is stored permuted
        for _ in range(steps):
            sim.step(1, fixed_dt=f["fixed_dt"])
        st = sim.download()
        hw = window_of(st)
        for kw in (dict(), dict(axes=(0, 2), center=(0.1 * hw, -0.2 * hw), depth=(-0.3 * hw, 0.4 * hw))):
            want, _ = array_project(nsc, sim, f, f["d"], hw, (33, 17), **kw)
            got = sim.project(hw, (33, 17), d=f["d"], **kw)
            assert same_maps(got, want), (steps, kw)
            assert got["pairs"] > 0 and got["count"].max() > 1
            assert same_maps(sim.project(hw, (33, 17), d=f["d"], **kw), got)       # repeated: the same bits
    # d=None: the d remembered from length_scale(apply=True); sizes stay the step's radii, as sample() reads them
    with pytest.raises(ValueError, match="remembered"):
        sim.project(hw, 16)
    ls = sim.length_scale(40, 8.0)
    want, _ = array_project(nsc, sim, f, ls["d"], hw, (16, 16))
    assert same_maps(sim.project(hw, 16), want)
    # the driver's window
    hw_drv = float(np.sqrt(ls["max_dist"] * 11 / 9))
    want, _ = array_project(nsc, sim, f, ls["d"], hw_drv, (24, 24))
    assert same_maps(sim.project(hw_drv, 24), want)


def test_stars_in_the_window(nsc):
    sim, f = make_sim(TWO_PHASE, steps=2)
    st = sim.download()
    hw = 0.6 * window_of(st)
    depth = (-0.5 * hw, 0.7 * hw)
    res = sim.project(hw, 8, d=f["d"], center=(0.1 * hw, 0.0), depth=depth, fields=("count",), stars=True)
    p = st["points"]
    keep = (sim._ptype == 1) & (np.abs(p[:, 1] - 0.1 * hw) <= hw) & (np.abs(p[:, 2]) <= hw) & (p[:, 0] >= depth[0]) & (p[:, 0] < depth[1])
    ids = np.flatnonzero(keep)
    assert np.count_nonzero(sim._ptype == 1) > ids.size > 0, "the window keeps some stars and drops some"
    assert np.array_equal(res["star_ids"], ids) and same_bits(res["star_uv"], np.ascontiguousarray(p[ids][:, 1:]))
    assert same_bits(res["star_mass"], f["mass"][ids].astype(np.float64))
    assert set(res) == {"count", "skipped", "pairs", "star_ids", "star_uv", "star_mass"}


def snapshot(sim):
    st = sim.download()
    comp = sim.download_composition()
    return [st[k] for k in sorted(st) if isinstance(st[k], np.ndarray)] + [comp[k] for k in sorted(comp)]


def test_twins_differing_only_in_project_calls(nsc):
    """project() between steps - alone, and alternating with sample() and census() on the one context - leaves download()'s
    bits what they are without it."""
    sim, f = make_sim(SMALL, forms="loop")
    twin, _ = make_sim(SMALL, forms="loop")
    both, _ = make_sim(SMALL, forms="loop")
    q = None
    for step in range(4):
        for s_ in (sim, twin, both):
            s_.step(1, fixed_dt=f["fixed_dt"])
        hw = window_of(sim.download())
        sim.project(hw, (33, 17), d=f["d"])
        sim.project(hw / 3, 16, d=f["d"], axes=(2, 0))
        if q is None:
            g = np.linspace(-hw, hw, 9)
            q = np.stack(np.meshgrid([0.0], g, g, indexing="ij"), axis=-1).reshape(-1, 3)
        both.sample(q, f["d"])
        both.project(hw, (17, 33), d=f["d"])
        both.census(f["mu_specie"])
        both.project(hw, 16, d=f["d"], depth=(-hw / 2, hw / 2))
        both.sample(q, f["d"])
    want = snapshot(twin)
    for s_ in (sim, both):
        got = snapshot(s_)
        assert len(got) == len(want) and all(same_bits(a, b) for a, b in zip(got, want))


def test_refusals_and_timing_keys(nsc):
    import ctypes as C
    from sph_code_amd import _lib
    from sph_code_amd._lib import dp, ip
    case = mc.CASES["subset-n257"]
    for kw in (dict(axes=(1, 1)), dict(axes=(0, 3)), dict(axes=(-1, 2)), dict(half_width=0.0), dict(half_width=(1.0, -1.0)),
               dict(half_width=np.inf), dict(half_width=np.nan), dict(npix=0), dict(npix=(4, 0)), dict(depth=(1.0, 1.0)),
               dict(depth=(2.0, 1.0)), dict(depth=(np.nan, 1.0)), dict(center=(np.nan, 0.0)), dict(npix=(1 << 15, 1 << 14))):
        with pytest.raises(ValueError):
            call(nsc, case, **kw)
    with pytest.raises(ValueError, match="unknown field"):
        call(nsc, case, fields=("density",))
    # a refused call writes nothing
    s = case["state"]
    c_ = nsc.context()
    img = np.full((4, 4), -7.0)
    one = np.full(1, -7, dtype=np.int64)
    ax, np_ = np.array([1, 1], dtype=np.int32), np.array([4, 4], dtype=np.int32)
    c32 = lambda a: a.ctypes.data_as(_lib.c_int32_p)
    rc = c_.lib.sphx_project_maps(c_.h, 257, dp(s["points"]), dp(s["mass"]), dp(s["particle_type"]), dp(s["sizes"]), dp(s["T"]), s["d"],
                                  c32(ax), dp(np.zeros(2)), dp(np.ones(2)), c32(np_), None, dp(img), None, None, None, None, ip(one), ip(one))
    assert rc == -1 and np.all(img == -7.0) and one[0] == -7
    # the resident call before a state, and before the first step
    ctx = _lib.Context()
    ax = np.array([1, 2], dtype=np.int32)
    assert ctx.lib.sphx_state_project(ctx.h, 1.0, c32(ax), dp(np.zeros(2)), dp(np.ones(2)), c32(np_), None, dp(img), None, None, None, None,
                                      None, None) == _lib.SPHX_E_STATE
    ctx.close()
    sim, f = make_sim(SMALL)
    with pytest.raises(RuntimeError, match="before the first"):
        sim.project(1.0, 4, d=f["d"])
    sim.step(1, fixed_dt=f["fixed_dt"])
    with pytest.raises(ValueError):
        sim.project(1.0, 4, d=f["d"], axes=(2, 2))
    sim.project(window_of(sim.download()), 4, d=f["d"])
    t = sim.map_timing()
    assert tuple(t) == nsc.MAP_STAGES == ("footprints", "count_scan", "list_build", "tiles", "read_back")
    assert all(v >= 0 for v in t.values()) and t["tiles"] > 0
    from sph_code_amd.multigpu import DistributedSim
    with pytest.raises(NotImplementedError):
        DistributedSim.project(None)
    del C
