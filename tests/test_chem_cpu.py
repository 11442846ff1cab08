"""chem_oracle - the NumPy restatement of chemisputtering_2 (nsc:1265-1416) - against the reference's own captured
results (tests/golden/chem_sphere_dust_n2048_k40.npz), the round model against the sequential order, the conditions on
every input set the GPU tests use, and the drop-in's boundary.

Measured, restatement against the reference's capture: mass_new equal bit for bit; f_un_new equal on all but 179 of 30720
elements - gas counts that are what is left of a cancellation (1e-9 of their row) - worst 1.07e-11 relative, 6.1e-4 of
the bound there.  The round model ends on the sequential counts bit for bit on every input set; the fixture takes 13
rounds, the hub 65 (its 64 rows + 1).
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import chem_fixture
import chem_oracle
from conftest import ROOT

SETS = list(chem_fixture.input_sets())


def test_oracle_reproduces_the_reference():
    f, o = chem_fixture.built("fixture")
    for nm in chem_oracle.OUTPUTS:
        ref = f["ref_" + nm]
        print(nm, "differing elements %d of %d, worst |diff| / |ref| %.2e, / bound %.2e" % (
            int(np.count_nonzero(o[nm] != ref)), ref.size, chem_oracle.worst_ratio(o[nm], ref, np.abs(ref)),
            chem_oracle.worst_ratio(o[nm], ref, o[nm + "_bound"])))
    assert np.array_equal(o["mass_new"], f["ref_mass_new"])
    chem_oracle.assert_within("f_un_new", o["f_un_new"], f["ref_f_un_new"], o["f_un_new_bound"])
    assert np.count_nonzero(o["f_un_new"] != f["ref_f_un_new"]) < 0.01 * o["f_un_new"].size
    # first-order bounds, not rtols: tight except on the few counts that are what is left of a cancellation
    for nm in chem_oracle.OUTPUTS:
        nz = o[nm] != 0.0
        rel = o[nm + "_bound"][nz] / np.abs(o[nm][nz])
        print(nm, "relative bound: median %.2e, worst %.2e" % (np.median(rel), rel.max()))
        assert np.median(rel) <= 1e-11, nm


def test_fixture_is_not_trivial():
    """Conditions on the inputs (a regenerated fixture that fails one changes its seed)."""
    f, o = chem_fixture.built("fixture")
    c = o["counts"]
    dusty, gas = f["particle_type"] == 2, f["particle_type"] == 0
    assert c["rows"] == int(dusty.sum()) == 102 and c["clamp1"] > 0 and c["clamp2"] > 0 and c["rounds"] >= 3
    assert c["columns_corrected"] > 0
    rel = np.abs(f["ref_mass_new"] / f["mass"] - 1.0)
    assert rel[dusty].max() > 1e-4 and rel[gas].max() > 1e-6 and np.all(rel[f["particle_type"] == 1] < 1e-12)
    assert np.all(f["ref_f_un_new"] >= 0.0) and np.allclose(np.sum(f["ref_f_un_new"], axis=1), 1.0, rtol=1e-12)
    assert np.array_equal(f["ref_f_un_new"][:, :6] > 0, f["f_un"][:, :6] > 0)


@pytest.mark.parametrize("name", SETS)
def test_round_model_ends_on_the_sequential_counts_and_no_decision_is_within_reach_of_the_bound(name):
    """chem_fixture.built runs the round model beside the sequential sweep and asserts equal bits (chem_oracle.sputter,
    model=True).  Every discrete decision of the set lies at least SLACK times the bound's size there away from its
    threshold: the library decides as the restatement does, its counts are equal, and the comparison leaves no element
    out."""
    f, o = chem_fixture.built(name)
    c = o["counts"]
    print(name, c, "slack", o["slack"])
    assert 1 <= c["rounds"] <= c["rows"] + 1
    assert set(o["slack"]) == set(chem_oracle.DECISIONS)
    for what, v in o["slack"].items():
        assert v >= chem_fixture.SLACK, (name, what, v)
    assert np.all(np.isfinite(o["mass_new"])) and np.all(np.isfinite(o["f_un_new"]))


def test_sets_reach_the_regimes_they_are_named_for():
    c = chem_fixture.built("module dt")[1]["counts"]
    assert c["clamp1"] == c["clamp2"] == c["clamp3"] == c["columns_corrected"] == 0 and c["rounds"] == 2, c
    f, o = chem_fixture.built("module dt")
    rel = np.abs(o["mass_new"] / f["mass"] - 1.0)[f["particle_type"] == 2]
    assert 1e-6 < rel.max() < 1e-4, rel.max()
    c = chem_fixture.built("hub")[1]["counts"]
    assert c["rows"] == c["pairs"] == chem_fixture.HUB_ROWS and c["rounds"] == c["rows"] + 1 and c["clamp1"] >= c["rows"], c
    c = chem_fixture.built("negative")[1]["counts"]
    assert c["clamp2"] > 0 and c["clamp3"] > 0 and c["columns_corrected"] > 0, c
    for name in ("no dust", "all dust", "no gas"):
        f, o = chem_fixture.built(name)
        assert o["counts"]["rows"] == o["counts"]["pairs"] == 0, name
        assert np.allclose(o["mass_new"], f["mass"], rtol=1e-14, atol=0.0), name
    f, o = chem_fixture.built("overflow")
    R = o["rows"]
    assert np.mean(R["F"][R["contributes"]][:, 7:] == 1.0) > 0.9            # exp overflow: inf / inf = NaN -> F = 1
    iterating = [n for n in SETS if chem_fixture.built(n)[1]["counts"]["rounds"] >= 3]
    print("sets that need iteration:", iterating)
    assert len(iterating) >= 15


def test_small_shapes_cover_the_sizes():
    names = [n for K in chem_fixture.CLOUD_K for n, _ in chem_fixture.shape_specs(K)]
    assert len(names) == len(set(names)) == 20
    for N in chem_fixture.CLOUD_N:
        assert sum(("n=%d " % N) in n for n in names) == 4
    for S in chem_fixture.CLOUD_S:
        assert any(n.endswith("S=%d" % S) for n in names)


def test_missing_entries_contribute_nothing():
    f = chem_fixture.short_cloud(5, 7)
    n = f["points"].shape[0]
    assert np.any(f["neighbor"] == n)
    o = chem_fixture.run_oracle(f, model=False)
    o2 = chem_fixture.run_oracle(dict(f, neighbor=f["neighbor"][:, :n]), model=False)
    for nm in chem_oracle.OUTPUTS:
        assert np.array_equal(o[nm], o2[nm]), nm
    assert o["counts"] == o2["counts"] and o["counts"]["pairs"] > 0


def test_compat_defaults_are_the_reference_s_module_values():
    import sph_code_amd.compat as nsc
    f = chem_fixture.load()
    assert np.array_equal(nsc.mu_specie, f["mu_specie"]) and np.array_equal(nsc.mineral_densities, f["mineral_densities"])
    assert np.array_equal(nsc.sputtering_yields, f["sputtering_yields"]) and np.array_equal(nsc.mrn_constants, f["mrn"])
    assert (nsc.k, nsc.amu, nsc.m_0) == (f["k_B"], f["amu"], f["m_0"]) == (chem_oracle.K_B, chem_oracle.AMU, chem_oracle.M_0)
    assert nsc.dt_0 == chem_oracle.DT_0 and nsc.CHEM_COUNTS == chem_oracle.COUNTS
    for a, b in zip(chem_oracle.tables(15), (nsc.mu_specie, nsc.mineral_densities, nsc.sputtering_yields)):
        assert np.array_equal(a, b)
    assert np.array_equal(nsc.chem_table(7, None, "mu_specie"), nsc.mu_specie[:7])
    with pytest.raises(ValueError):
        nsc.chem_table(32, None, "mu_specie")
    with pytest.raises(ValueError):
        nsc.chem_table(15, np.ones(14), "sputtering_yields")


def test_header_declares_and_library_exports_chemisputtering_2():
    src = open(os.path.join(ROOT, "include", "sphx.h")).read()
    body = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for nm in ("sphx_chemisputtering_2", "sphx_chem_last_timing"):
        assert re.search(r"\bint\s+%s\s*\(" % nm, body), nm
    for quirk in ("mu_array (the input)", "He++ column", "normalised twice", "(e-) is computed", "inf / inf = NaN",
                  "not clamped again", "distinct"):
        assert quirk in src, quirk
    import sph_code_amd._lib as L
    lib = ctypes.CDLL(L.LIB_PATH)
    assert hasattr(lib, "sphx_chemisputtering_2") and hasattr(lib, "sphx_chem_last_timing")
    assert len(L.SIGNATURES["sphx_chemisputtering_2"][1]) == 24


def test_compat_signature_is_the_reference_s():
    import sph_code_amd.compat as nsc
    names = list(inspect.signature(nsc.chemisputtering_2).parameters)
    assert names[:8] == ["points", "neighbor", "mass", "f_un", "mu_array", "sizes", "T", "particle_type"]
    assert names[8:] == ["d", "dt", "mu_specie", "mineral_densities", "sputtering_yields", "mrn_constants", "full"]
    assert callable(nsc.chem_last_timing)
