"""rad_oracle - the NumPy restatement of rad_heating's lines 922-965 - against the reference's own captured results
(tests/golden/rad_<case>.npz), and the semantics the GPU tests then hold libsphx to.

Worst differences measured, restatement against the reference's capture (both cases, line mode):
    blocked        0 ulp (bit for bit)       star_distance  0 ulp (bit for bit)
    lum_factor     0 (bit for bit)           extinction     4.3e-16 relative (0.24 of its 8 ulp bound)
    lf2            6.2e-16 relative (1.5e-4 of its bound)
    momentum       8.4e-15 relative, where the sources' pulls cancel (1.3e-4 of its bound, a bound on sum|term|)
    smallest margin of the fixtures: 5.4e-6 (line), 8.6e-7 (segment); the condition is margin > 1e-9.
"""
import numpy as np
import pytest

import rad_fixture
import rad_oracle

EPS = 2.0 ** -52


def ulps(x, ref):
    with np.errstate(all="ignore"):
        return np.abs(x - ref) / (EPS * np.abs(ref))


@pytest.mark.parametrize("case", rad_fixture.CASES)
def test_fixture_margin(case):
    """A condition on the inputs: no (particle, ray) pair of the fixture sits on a column's edge (if a regenerated
    fixture fails this, its seed changes, not the threshold)."""
    for mode in rad_oracle.MODES:
        m = rad_fixture.oracle(case, mode)["margin"]
        print(case, mode, "margin %.3e" % m)
        assert m > rad_fixture.MIN_MARGIN, (case, mode, m)


@pytest.mark.parametrize("case", rad_fixture.CASES)
def test_oracle_reproduces_the_reference(case):
    f = rad_fixture.load(case)
    o = rad_fixture.oracle(case, "line")
    assert f["W6_constant"] == rad_oracle.C2 and f["solar_luminosity"] == rad_oracle.SOLAR_LUMINOSITY
    assert f["c"] == rad_oracle.C_LIGHT
    for nm in ("blocked", "star_distance"):
        u = ulps(o[nm], f["ref_" + nm])
        u = u[o[nm] != f["ref_" + nm]]
        print(case, nm, "worst %.1f ulp" % (u.max() if u.size else 0.0))
        assert o[nm].shape == f["ref_" + nm].shape
        assert not u.size or u.max() <= 4.0, (case, nm, u.max())
    for nm in ("lum_factor", "extinction", "lf2", "momentum"):
        print(case, nm, "worst |diff| / |ref| %.2e, / bound %.2e" % (
            rad_oracle.worst_ratio(o[nm], f["ref_" + nm], np.abs(f["ref_" + nm])),
            rad_oracle.worst_ratio(o[nm], f["ref_" + nm], o[nm + "_bound"])))
        rad_oracle.assert_within(nm, o[nm], f["ref_" + nm], o[nm + "_bound"], case)
    # the bounds are first-order bounds of 1e-12 sums, not rtols: the exponent's factor is in them
    assert np.all(o["lf2_bound"] <= 1e-8 * np.abs(o["lf2"]) + 1e-300)
    assert o["lum_factor"].max() > 10.0


@pytest.mark.parametrize("case", rad_fixture.CASES)
def test_segment_column_never_exceeds_the_line_column(case):
    line, seg = rad_fixture.oracle(case, "line"), rad_fixture.oracle(case, "segment")
    assert np.all(seg["blocked"] <= line["blocked"])
    assert np.any(seg["blocked"] < line["blocked"])
    assert np.array_equal(seg["star_distance"], line["star_distance"])


@pytest.mark.parametrize("case", rad_fixture.CASES)
def test_segment_columns_add_along_a_ray(case):
    """b on the segment a -> c at a dyadic fraction: column(a -> c) = column(a -> b) + column(b -> c)."""
    f = rad_fixture.load(case)
    part = (f["positions"], f["sizes"], f["masses"], f["mu_array"], f["cross_array"])
    checked = 0
    for s in range(f["sources"].shape[0]):
        for q in range(0, f["targets"].shape[0], 3):
            a, c = f["sources"][s], f["targets"][q]
            for frac in (3.0 / 8.0, 0.5):
                b = a + frac * (c - a)
                ac = rad_oracle.columns(*part, a[None], c[None], mode="segment", amu=f["amu"])
                ab = rad_oracle.columns(*part, a[None], b[None], mode="segment", amu=f["amu"])
                bc = rad_oracle.columns(*part, b[None], c[None], mode="segment", amu=f["amu"])
                if min(ac["margin"], ab["margin"], bc["margin"]) <= rad_fixture.MIN_MARGIN:
                    continue                                   # (a particle's foot point sits on b: another ray)
                whole, parts = ac["blocked"][0, 0], ab["blocked"][0, 0] + bc["blocked"][0, 0]
                assert abs(whole - parts) <= rad_oracle.TAU * whole, (case, s, q, frac, whole, parts)
                checked += 1
    assert checked >= 8


def small_cloud():
    rs = np.random.RandomState(7)
    n = 40
    pos = rs.rand(n, 3) * 1e17
    pt = np.zeros(n); pt[[3, 9]] = 1.0; pt[[5, 6]] = 2.0
    return dict(positions=pos, ptypes=pt, masses=1e30 * (1 + rs.rand(n)), sizes=2e16 * (1 + rs.rand(n)),
                cross=10.0 ** rs.uniform(-25, -21, n), mu=2.0 + rs.rand(n), sources=pos[[3, 9]].copy(),
                lum=np.array([1.0, 30.0]), targets=pos[[0, 11, 20]].copy(), dt=7.9e12)


def run(c, **kw):
    a = dict(c)
    a.update(kw)
    return rad_oracle.transfer(a["positions"], a["ptypes"], a["masses"], a["sizes"], a["cross"], a["mu"], a["sources"],
                               a["lum"], a["targets"], a["dt"], mode=a.get("mode", "line"))


def test_degenerate_ray_zeroes_its_source():
    c = small_cloud()
    t = c["targets"].copy()
    t[1] = c["sources"][0]                                     # ray (0, 1): source == target
    o = run(c, targets=t)
    assert o["blocked"][0, 1] == 0.0 and o["star_distance"][0, 1] == 0.0
    assert np.all(o["lum_factor"][0] == 0.0)                   # its 0/0 reaches every particle through nan_to_num
    assert np.any(o["lum_factor"][1] > 0.0)
    assert np.all(np.isfinite(o["lf2"]))


def test_no_targets_no_sources_no_gas():
    c = small_cloud()
    G = int(np.count_nonzero(c["ptypes"] != 1))
    o = run(c, targets=np.zeros((0, 3)))
    assert o["blocked"].shape == (2, 0) and o["lum_factor"].shape == (2, G) and np.all(o["lum_factor"] == 0.0)
    assert np.all(o["lf2"] > 0.0)                              # unattenuated: exp(0)
    o = run(c, sources=np.zeros((0, 3)), lum=np.zeros(0))
    assert o["blocked"].shape == (0, 3) and o["lum_factor"].shape == (0, G)
    assert np.all(o["lf2"] == 0.0) and np.all(o["momentum"] == 0.0) and np.all(o["extinction"] > 0.0)
    pt = c["ptypes"].copy()
    pt[pt == 0] = 2.0
    with pytest.raises(ValueError):
        run(c, ptypes=pt)


def test_segment_end_particles_are_decided_exactly():
    """A particle AT the source blocks its ray, one AT the target does not (half-open), whatever the rounding."""
    c = small_cloud()
    line, seg = run(c), run(c, mode="segment")
    w = rad_oracle.weights(c["sizes"], c["masses"], c["mu"], c["cross"])
    part = (c["positions"], c["sizes"], c["masses"], c["mu"], c["cross"])
    one = rad_oracle.columns(part[0][[3, 0]], part[1][[3, 0]], part[2][[3, 0]], part[3][[3, 0]], part[4][[3, 0]],
                             c["sources"][:1], c["targets"][:1], mode="segment")
    assert one["blocked"][0, 0] == w[3]                        # the source star itself, not the target particle
    assert np.all(seg["blocked"] <= line["blocked"])
