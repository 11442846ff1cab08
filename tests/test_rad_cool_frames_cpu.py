"""The transformed rad and cool cases of tests/rad_cool_frames.py are sound, shown with the NumPy restatements alone (no
GPU): the shifts and scalings are exact, a shifted oracle result is the base's bit for bit, scaled columns obey their exact
power of two, every rad case keeps its margin from a column's edge, and no case is vacuous - lf2 and momentum are non-zero
where they are compared, the cool energy is non-zero on the gas, scale_up is in the linear regime and half_capped between
the two."""
import numpy as np
import pytest

import cool_oracle
import rad_cool_frames as rcf
import rad_fixture
import rad_oracle

RAD_EXACT = [c for c in rcf.RAD_CASES if c[1] in rcf.SHIFTS + rcf.SCALES]
COOL_EXACT = [c for c in rcf.COOL_CASES if c[1] in rcf.SHIFTS + rcf.SCALES + ("half_capped",)]


def _on_lattice(p, q):
    k_ = np.round(p / q)
    return np.array_equal(k_ * q, p) and np.abs(k_).max() <= 2 ** rcf.Q_BITS


@pytest.mark.parametrize("case", RAD_EXACT, ids=rcf.case_id)
def test_rad_shift_and_scale_frames_are_exact(case):
    f, meta = rcf.rad_case(*case)
    base, sc, off = meta["base"], meta["scale"], meta["offset"]
    for key in ("positions", "sources", "targets"):
        assert _on_lattice(base[key], meta["q"]), key
        assert np.array_equal((f[key] - off) / sc, base[key]), key
    assert np.array_equal(f["sizes"] / sc, base["sizes"])
    # every difference the operation forms is the base's, bit for bit (times the scale)
    i = np.random.RandomState(2).randint(0, len(base["positions"]), 4000)
    for a in ("sources", "targets"):
        for r in range(min(3, len(base[a]))):
            assert np.array_equal(f["positions"][i] - f[a][r], (base["positions"][i] - base[a][r]) * sc)
    assert np.array_equal(f["targets"][0] - f["sources"][0], (base["targets"][0] - base["sources"][0]) * sc)
    # sources and targets are particles of the snapped cloud
    for a in ("sources", "targets"):
        assert all(np.any(np.all(f["positions"] == x, axis=1)) for x in f[a][:5])


@pytest.mark.parametrize("mode", rad_oracle.MODES)
@pytest.mark.parametrize("case", rcf.RAD_CASES, ids=rcf.case_id)
def test_rad_case_is_sound(case, mode):
    """The margin of every case; shifted results equal to the base's bit for bit; scaled columns by the exact power of
    two; lf2 and momentum non-zero on at least half the non-star particles wherever they are compared."""
    name, frame = case
    f, meta = rcf.rad_case(*case)
    o, ob = rcf.rad_reference(name, frame, mode), rcf.rad_reference(name, None, mode)
    sc = meta["scale"]
    print("%s %s: margin %.3g (base %.3g)" % (rcf.case_id(case), mode, o["margin"], ob["margin"]))
    assert o["margin"] > rad_fixture.MIN_MARGIN and ob["margin"] > rad_fixture.MIN_MARGIN
    assert np.all(np.isfinite(o["blocked"])) and np.all(o["blocked"] > 0.0) and np.all(o["star_distance"] > 0.0)
    if frame in rcf.SHIFTS:
        assert o["margin"] == ob["margin"]
        for nm in rad_oracle.OUTPUTS:
            assert np.array_equal(o[nm], ob[nm], equal_nan=True), nm
    if frame in rcf.SCALES:
        assert o["margin"] == ob["margin"]
        assert np.array_equal(o["blocked"] * sc ** 2, ob["blocked"])
        assert np.array_equal(o["star_distance"] / sc, ob["star_distance"])
    if frame in rcf.COLUMNS_ONLY:
        assert "lf2" not in o and np.array_equal(o["w"][f["ptypes"] != 1] * sc ** 2, ob["extinction"])
        return
    if frame in rcf.SCALES:
        assert np.array_equal(o["extinction"] * sc ** 2, ob["extinction"])
    G = int(np.count_nonzero(f["ptypes"] != 1))
    assert o["lf2"].shape == (G,) and np.all(np.isfinite(o["lf2"])) and np.all(np.isfinite(o["momentum"]))
    assert np.count_nonzero(o["lf2"]) >= 0.5 * G
    assert np.count_nonzero(np.any(o["momentum"] != 0.0, axis=1)) >= 0.5 * G      # (a plane: no z component)
    assert np.count_nonzero(o["lum_factor"]) >= 0.5 * o["lum_factor"].size
    if mode == "segment":
        assert np.any(o["blocked"] < rcf.rad_reference(name, frame, "line")["blocked"])


@pytest.mark.parametrize("name", rad_fixture.CASES)
def test_rad_scale_down_deposits_nothing(name):
    """Why scale_down is a columns-only case: at 2^-57 the one metre of nsc:941 dwarfs every distance, lum_factor ~ 1e37
    and lf2 and momentum are exactly 0 on every particle - a comparison of them would compare zeros."""
    f, _ = rcf.rad_case(name, "scale_down")
    o = rad_oracle.transfer(*rad_fixture.transfer_args(f), **rad_fixture.constants(f))
    assert np.all(o["lf2"] == 0.0) and np.all(o["momentum"] == 0.0) and np.max(o["lum_factor"]) > 1e30


def test_rad_large_clouds_have_the_shape_they_are_for():
    """Five sources and thirteen targets on N = 8193 and 20011, and one case of one ray more than a workgroup holds."""
    for name, (n, n_src, n_dst, _) in rcf.RAD_LARGE.items():
        f = rcf.rad_base(name)[0]
        n_dst = rcf.wg_rays() + 1 if n_dst is None else n_dst
        assert f["positions"].shape == (n, 3) and f["sources"].shape == (n_src, 3) and f["targets"].shape == (n_dst, 3)
        assert np.count_nonzero(f["ptypes"] == 1) == len(rcf.STAR_MASSES) and np.any(f["ptypes"] == 2)
        assert len(np.unique(f["positions"], axis=0)) == n
    assert rcf.rad_base("two_phase_n20011_wide")[0]["targets"].shape[0] * 1 == rcf.wg_rays() + 1


@pytest.mark.parametrize("case", COOL_EXACT, ids=rcf.case_id)
def test_cool_shift_and_scale_frames_are_exact(case):
    c, meta = rcf.cool_case(*case)
    base, sc = meta["base"], meta["scale"]
    assert _on_lattice(base["positions"], meta["q"])
    assert np.array_equal((c["positions"] - meta["offset"]) / sc, base["positions"]) and c["d"] / sc == base["d"]
    assert c["neighbor"] is base["neighbor"]
    nb = base["neighbor"]
    j = np.random.RandomState(3).randint(0, nb.shape[0], 4000)
    p = nb[j, np.random.RandomState(4).randint(0, nb.shape[1], 4000)]
    assert np.array_equal(c["positions"][p] - c["positions"][j], (base["positions"][p] - base["positions"][j]) * sc)


@pytest.mark.parametrize("case", rcf.COOL_CASES, ids=rcf.case_id)
def test_cool_case_is_sound(case):
    """Finite everywhere, the base's live rows, energy non-zero on at least half the gas; shifted results equal to the
    base's bit for bit; scale_up linear, half_capped between the regimes."""
    name, frame = case
    c, meta = rcf.cool_case(*case)
    o, ob = rcf.cool_reference(name, frame), rcf.cool_reference(name, None)
    gas = c["particle_type"] == 0
    share = rcf.capped_share(o)
    print("%s: capped share %.3f, max rec_array[5] %.3g, %d live rows" % (rcf.case_id(case), share, o["rec_array"][5].max(),
                                                                        o["row_contributes"].sum()))
    for nm in cool_oracle.OUTPUTS:
        assert np.all(np.isfinite(o[nm])) and np.all(np.isfinite(o[nm + "_bound"])), nm
    assert np.array_equal(o["row_contributes"], ob["row_contributes"]) and o["row_contributes"].sum() >= 0.8 * gas.sum()
    assert np.count_nonzero(o["energy"][gas]) >= 0.5 * gas.sum()
    if frame in rcf.SHIFTS:
        for nm in cool_oracle.OUTPUTS:
            assert np.array_equal(o[nm], ob[nm]), nm
    if frame == "scale_up":
        assert o["rec_array"][5].max() < 0.5
    if frame == "half_capped":
        assert 4 <= rcf.HALF_CAPPED_EXP[name] <= 20 and 0.2 <= share <= 0.8
    if frame == "line":
        p = c["positions"]
        same = len(p) - len(np.unique(p[:, 0]))
        print("%s: %d particles on top of another" % (rcf.case_id(case), same))
        assert np.all(p[:, 1:] == 0.0) and (same > 0 or len(p) < 8193)


def test_cool_bases_start_in_the_capped_regime():
    """What the scale frames are for: the bases themselves sit at the 0.9999 cap on four particles in five."""
    for name in rcf.COOL_BASES:
        assert rcf.capped_share(rcf.cool_reference(name, None)) > 0.75
