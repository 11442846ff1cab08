"""The closing block of the time loop (code_running.py:493-540) without a GPU: the NumPy restatement tests/scale_oracle.py
against the fixtures the driver's own lines produced (tests/golden/make_golden_scale.py), the two-order-statistics form
of the percentile against np.percentile, and the library's host-side finish (sphx_length_scale_finish: the lerp and the
two pow calls, which need no device) against the restatement - all bit for bit."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
import scale_oracle as so

CASES = ("scale_a", "scale_b")
M_VALUES = list(range(1, 70)) + [255, 256, 257, 1000, 4097, 20011]


@pytest.mark.parametrize("name", CASES)
def test_restatement_has_the_driver_block_bits(name):
    g = load_golden(name)
    ls = so.length_scale(g["points"], g["velocities"], int(g["N_INT_PER_PARTICLE"]))
    assert ls["n_slow"] == int(g["out_n_slow"])
    assert so.same_bits(ls["max_dist"], g["out_max_dist"])
    assert so.same_bits(ls["d"], g["out_d"]) and so.same_bits(ls["d"], g["out_nsc_d"])
    ad = so.adapt_sizes(g["neighbor"], g["densities"], g["densities_0"], g["sizes"], g["particle_type"], ls["d"], float(g["raise_factor"]))
    np.testing.assert_array_equal(ad["exp_neighbor_count"], g["out_exp_neighbor_count"])
    np.testing.assert_array_equal(ad["num_nontrivial"], g["num_nontrivial"])
    assert so.same_bits(ad["new_smoothing"], g["out_new_smoothing"])
    assert so.same_bits(ad["sizes"], g["out_sizes"])
    assert so.same_bits(g["out_densities_0"], g["densities"])                  # drv:540
    assert ad["counts"]["missing"] == int(np.count_nonzero(g["neighbor"] == g["neighbor"].shape[0]))


def test_fixtures_cover_both_branches_and_every_type():
    a, b = load_golden("scale_a"), load_golden("scale_b")
    assert a["densities_0"].shape == a["densities"].shape and b["densities_0"].shape != b["densities"].shape
    assert np.all(b["out_new_smoothing"] == 1.0) and not np.all(a["out_new_smoothing"] == 1.0)
    for g in (a, b):
        n = g["points"].shape[0]
        assert n <= 2048
        assert set(np.unique(g["particle_type"])) == {0.0, 1.0, 2.0}
        fast = 1.0 - float(g["out_n_slow"]) / n
        assert 0.05 < fast < 0.2
    ad = so.adapt_sizes(a["neighbor"], a["densities"], a["densities_0"], a["sizes"], a["particle_type"], float(a["out_d"]), float(a["raise_factor"]))
    assert ad["counts"]["bonus"] > 0 and ad["counts"]["capped"] > 0 and ad["counts"]["nan_to_num"] > 0


def _values(M, kind, rng):
    v = np.exp(rng.normal(size=M) * 3.0)
    if kind == "ties":
        v = np.round(v * 2.0) / 2.0
    if kind == "inf":
        v[rng.randint(0, M, size=max(1, M // 8))] = np.inf
    return v


@pytest.mark.parametrize("kind", ("plain", "ties", "inf"))
def test_two_order_statistics_are_np_percentile(kind):
    rng = np.random.RandomState(7)
    for M in M_VALUES:
        v = _values(M, kind, rng)
        with np.errstate(all="ignore"):
            want = np.percentile(v, 90.)
            lo, hi, a, b, got = so.two_stat_percentile(v, np.true_divide(90., 100))
        assert so.same_bits(got, want), (kind, M, got, want)
        s = np.sort(v)
        assert a == s[lo] and b == s[hi] and hi in (lo, lo + 1)


def test_nan_among_the_values_gives_nan():
    v = np.array([3.0, np.nan, 1.0, 2.0])
    assert np.isnan(np.percentile(v, 90.)) and np.isnan(so.two_stat_percentile(v, 0.9)[4])


@pytest.mark.parametrize("kind", ("plain", "ties", "inf"))
def test_host_finish_has_the_restatement_bits(kind):
    """sphx_length_scale_finish from the exact order statistics: np.percentile's max_dist and the driver's d."""
    import sph_code_amd._lib as L
    lib = L.load_library()
    rng = np.random.RandomState(11)
    for M in M_VALUES:
        pts = np.zeros((M, 3))
        pts[:, 0] = np.sqrt(_values(M, kind, rng)) * 1e16
        with np.errstate(all="ignore"):
            ref = so.length_scale(pts, np.zeros((M, 3)), 40)
            md, d = C.c_double(), C.c_double()
            rc = lib.sphx_length_scale_finish(ref["n_slow"], ref["n_nan"], float(np.true_divide(90., 100)), ref["a"], ref["b"], 40.0, 0.9,
                                              C.cast(C.byref(md), L.c_double_p), C.cast(C.byref(d), L.c_double_p))
        assert rc == 0
        assert so.same_bits(md.value, ref["max_dist"]), (kind, M)
        assert so.same_bits(d.value, ref["d"]), (kind, M, d.value, ref["d"])


def test_host_finish_refuses_an_empty_selection():
    import sph_code_amd._lib as L
    lib = L.load_library()
    md, d = C.c_double(), C.c_double()
    assert lib.sphx_length_scale_finish(0, 0, 0.9, 1.0, 1.0, 40.0, 0.9, C.cast(C.byref(md), L.c_double_p), C.cast(C.byref(d), L.c_double_p)) == -1
    with pytest.raises(ValueError):
        so.length_scale(np.zeros((3, 3)), np.full((3, 3), 1e6), 40)
