"""GPU checks of chemisputtering_2 (nsc:1265-1416; include/sphx.h sphx_chemisputtering_2) against the NumPy restatement
tests/chem_oracle.py, to the bounds that module derives (1e-12 sum|term| per sum, 16 ulp per coefficient, the
cancellation of h^2 - r^2 near the edge of a support, exp and the K_u / L_u quotient to first order, the counts' bounds
carried through the ordered sweep and the closing correction).  No element is left out of any comparison, and the counts
are compared for equality except `rounds` (the library iterates in double, the model in longdouble: both end on their
sequential result, after a number of rounds that is bounded by the contributing rows + 1 and printed beside the
model's - a row whose spread-out sum happens to reproduce its unclamped loss bit for bit in one precision and not in
the other saves or costs a round): tests/test_chem_cpu.py shows that no decision of any input set used here lies within reach of the bound."""
import numpy as np
import pytest

import chem_fixture
import chem_oracle
import cool_fixture
import dust_fixture

pytestmark = pytest.mark.gpu

OUT = chem_oracle.OUTPUTS
EXACT = tuple(nm for nm in chem_oracle.COUNTS if nm != "rounds")


def kwargs(f):
    kw = {nm: f[nm] for nm in chem_fixture.TABLES}
    return dict(kw, d=f["d"], dt=f["dt"], mrn_constants=f.get("mrn"))


def gpu(f, **over):
    import sph_code_amd.compat as nsc
    a, b, c = nsc.chemisputtering_2(*chem_fixture.args(f), full=True, **dict(kwargs(f), **over))
    return dict(mass_new=a, f_un_new=b, counts=c)


def check(name, iterates=False):
    f, o = chem_fixture.built(name)
    got = gpu(f)
    for nm in OUT:
        print(name, nm, "worst |diff| / bound %.3g" % chem_oracle.worst_ratio(got[nm], o[nm], o[nm + "_bound"]))
    print(name, "counts", got["counts"], "restatement", o["counts"])
    for nm in OUT:
        chem_oracle.assert_within(nm, got[nm], o[nm], o[nm + "_bound"], name)
    for nm in EXACT:
        assert got["counts"][nm] == o["counts"][nm], (name, nm)
    assert 0 <= got["counts"]["rounds"] <= o["counts"]["rows"] + 1, name
    if iterates:                                                             # a set BUILT to need iteration
        assert got["counts"]["rounds"] >= 3, name
    return f, o, got


def test_fixture_and_the_reference_s_capture():
    f, o, got = check("fixture", iterates=True)
    c = got["counts"]
    assert c["clamp1"] > 0 and c["clamp2"] > 0 and c["columns_corrected"] > 0
    for nm in OUT:
        print("against the reference", nm, "worst |diff| / bound %.3g" % chem_oracle.worst_ratio(got[nm], f["ref_" + nm], o[nm + "_bound"]))
        chem_oracle.assert_within(nm, got[nm], f["ref_" + nm], o[nm + "_bound"], "reference")


def test_module_dt_nothing_clamped_two_rounds():
    f, o, got = check("module dt")
    c = got["counts"]
    assert c["clamp1"] == c["clamp2"] == c["clamp3"] == 0 and c["rounds"] == 2
    rel = np.abs(got["mass_new"] / f["mass"] - 1.0)[f["particle_type"] == 2]
    assert 1e-6 < rel.max() < 1e-4


@pytest.mark.parametrize("K", chem_fixture.CLOUD_K)
def test_small_shapes(K):
    """N = K + 1, around the workgroup size and over several workgroups; S = 7, 15, 32 in turn."""
    clamps = 0
    for name, _ in chem_fixture.shape_specs(K):
        clamps += check(name)[2]["counts"]["clamp1"]
    assert (clamps > 0) == (K > 1)


@pytest.mark.parametrize("name", ["no dust", "all dust", "no gas"])
def test_nothing_to_do(name):
    """No dust row, no gas entry: no reverse list, no round; the closing correction and the outputs still run."""
    f, o, got = check(name)
    c = got["counts"]
    assert c["rows"] == c["pairs"] == c["rounds"] == 0
    assert np.allclose(got["mass_new"], f["mass"], rtol=1e-14, atol=0.0)


@pytest.mark.parametrize("n,K", chem_fixture.SHORT)
def test_fewer_particles_than_columns(n, K):
    """Entries equal to N contribute nothing."""
    name = "short n=%d K=%d" % (n, K)
    f, o, got = check(name)
    assert n > K - 1 or np.any(f["neighbor"] == n)
    if n < K:
        again = gpu(dict(f, neighbor=np.ascontiguousarray(f["neighbor"][:, :n])))
        for nm in OUT:
            assert np.array_equal(got[nm], again[nm]), nm
        assert got["counts"] == again["counts"]


def test_hub_chain_as_deep_as_the_rows():
    """One gas particle in the list of 64 dust rows, a clamp in each: row j waits for row j - 1, one round per row."""
    f, o, got = check("hub", iterates=True)
    c = got["counts"]
    assert c["rows"] == chem_fixture.HUB_ROWS and c["clamp1"] >= c["rows"]
    assert c["rows"] // 2 < c["rounds"] <= c["rows"] + 1
    hub_before = f["f_un"][0, 7:] * f["mass"][0]
    # 1 % of 1 %, 64 times - in every column but silicon's, which the grains give to the gas
    assert np.count_nonzero(got["f_un_new"][0, 7:] * got["mass_new"][0] < 1e-100 * hub_before) == 7


def test_negative_compositions_clamps_2_and_3_and_the_closing_correction():
    f, o, got = check("negative")
    c = got["counts"]
    assert c["clamp2"] > 0 and c["clamp3"] > 0 and c["columns_corrected"] > 0
    assert np.any(f["f_un"] < 0.0) and np.all(got["f_un_new"][:, 6:] >= 0.0)


def test_exp_overflow_gives_f_sput_1():
    f, o, got = check("overflow")
    dusty = f["particle_type"] == 2
    assert np.allclose(got["mass_new"][dusty], f["mass"][dusty], rtol=1e-8, atol=0.0)


def test_same_bits_on_every_call_and_inputs_untouched():
    import sph_code_amd.compat as nsc
    f = chem_fixture.load()
    a_ = [np.array(a, copy=True) for a in chem_fixture.args(f)]
    keep = [np.array(a, copy=True) for a in a_]
    kw = kwargs(f)
    a = nsc.chemisputtering_2(*a_, full=True, **kw)
    b = nsc.chemisputtering_2(*a_, full=True, **kw)
    short = nsc.chemisputtering_2(*a_, **kw)
    assert len(a) == 3 and len(short) == 2 and a[2] == b[2]
    for x, y in zip(a[:2], b[:2]):
        assert np.array_equal(x, y)
    for x, y in zip(a[:2], short):
        assert np.array_equal(x, y)
    for x, y in zip(a_, keep):
        assert np.array_equal(x, y)
    # d and dt default to the module attributes, the tables to the module's
    nsc.d, nsc.dt = f["d"], f["dt"]
    try:
        dflt = nsc.chemisputtering_2(*a_)
    finally:
        nsc.d, nsc.dt = None, nsc.dt_0
    for x, y in zip(a[:2], dflt):
        assert np.array_equal(x, y)


def test_timing_keys():
    import sph_code_amd.compat as nsc
    gpu(chem_fixture.built("side call")[0])
    ms = nsc.chem_last_timing()
    assert list(ms) == ["upload", "rows", "reverse", "rounds", "closing"]
    assert all(v >= 0.0 for v in ms.values()) and ms["rounds"] > 0.0 and ms["rows"] > 0.0


def test_status_codes_of_the_c_abi():
    import sph_code_amd.compat as nsc
    from sph_code_amd._lib import dp, ip
    f = chem_fixture.cloud(64, 7, 15, 14)
    ctx = nsc.context()
    n, K, S = 64, 7, 15
    a = {k: np.ascontiguousarray(v) for k, v in f.items() if isinstance(v, np.ndarray)}
    mrn = np.array(nsc.mrn_constants, dtype=np.float64)
    mass_new, f_new = np.full(n, -7.0), np.full((n, S), -7.0)

    def call(n_=n, k_=K, s_=S, d=f["d"], dt=f["dt"], kB=nsc.k, amu=nsc.amu, m0=nsc.m_0, counts=None, **over):
        p = dict(pos=dp(a["points"]), nb=ip(a["neighbor"]), m=dp(a["mass"]), f=dp(a["f_un"]), mu=dp(a["mu_array"]), sz=dp(a["sizes"]),
                 T=dp(a["T"]), pt=dp(a["particle_type"]), mus=dp(a["mu_specie"]), dens=dp(a["mineral_densities"]),
                 ys=dp(a["sputtering_yields"]), mrn=dp(mrn), mn=dp(mass_new), fn=dp(f_new))
        p.update(over)
        return ctx.lib.sphx_chemisputtering_2(ctx.h, n_, k_, s_, p["pos"], p["nb"], p["m"], p["f"], p["mu"], p["sz"], p["T"], p["pt"], d, dt,
                                              p["mus"], p["dens"], p["ys"], p["mrn"], kB, amu, m0, p["mn"], p["fn"], counts)

    bad = [call(n_=0), call(n_=-1), call(k_=0), call(k_=65), call(s_=6), call(s_=33), call(d=np.inf), call(d=np.nan),
           call(dt=np.nan), call(dt=-np.inf), call(kB=np.nan), call(amu=np.inf), call(m0=np.nan), call(n_=2 ** 31 // 7 + 64)]
    bad += [call(**{nm: None}) for nm in ("pos", "nb", "m", "f", "mu", "sz", "T", "pt", "mus", "dens", "ys", "mrn", "mn", "fn")]
    for nm, at, v in (("mus", 3, np.nan), ("dens", 14, np.inf), ("ys", 0, np.nan)):
        t = a[{"mus": "mu_specie", "dens": "mineral_densities", "ys": "sputtering_yields"}[nm]].copy()
        t[at] = v
        bad.append(call(**{nm: dp(t)}))
    bad.append(call(mrn=dp(np.array([50e-10, np.nan]))))
    for rc in bad:
        assert rc == -1, rc                                                              # SPHX_E_ARG
    assert np.all(mass_new == -7.0) and np.all(f_new == -7.0)                             # nothing written
    assert ctx.lib.sphx_chemisputtering_2(None, n, K, S, *([None] * 8), 1.0, 1.0, *([None] * 4), 1.0, 1.0, 1.0, None, None, None) == -1
    assert call() == 0 and np.all(mass_new > 0.0)                                         # counts NULL
    counts = np.full(7, -7, dtype=np.int64)
    assert call(counts=ip(counts)) == 0 and np.all(counts >= 0) and counts[6] <= counts[0] + 1
    ms = np.zeros(5)
    assert ctx.lib.sphx_chem_last_timing(ctx.h, dp(ms)) == 0 and np.all(ms >= 0.0) and ms[1] > 0.0
    assert ctx.lib.sphx_chem_last_timing(ctx.h, None) == -1


def test_a_call_between_rad_cooling_and_supernova_destruction_leaves_their_bits():
    import sph_code_amd.compat as nsc
    c = cool_fixture.cloud(257, 7, 31)
    ca = cool_fixture.cloud_compat_args(c)
    df = dust_fixture.input_sets()["side call"]()
    f = chem_fixture.built("side call")[0]

    def dust():
        return nsc.supernova_destruction(*dust_fixture.args(df), full=True, **dust_fixture.opts(df))

    cool0, dust0 = nsc.rad_cooling(*ca, d=c["d"], full=True), dust()
    cool1 = nsc.rad_cooling(*ca, d=c["d"], full=True)
    mine = gpu(f)
    dust1 = dust()
    again = gpu(f)
    for x, y in zip(cool0, cool1):
        assert np.array_equal(x, y)
    assert dust0[2] == dust1[2]
    for x, y in zip(dust0[:2], dust1[:2]):
        assert np.array_equal(x, y)
    for nm in OUT:
        assert np.array_equal(mine[nm], again[nm]), nm
    assert mine["counts"] == again["counts"] and mine["counts"]["clamp1"] > 0
