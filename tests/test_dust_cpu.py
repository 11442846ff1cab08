"""dust_oracle - the NumPy restatement of supernova_destruction (nsc:1211-1263) - against the reference's own captured
results (tests/golden/dust_sphere_dust_n2048_k40.npz), the conditions on every input set the GPU tests use, and the
drop-in's boundary.

Measured, restatement against the reference's capture: frac_destruction equal bit for bit (each grain adds its rows in
the reference's order); frac_reuptake 3.0e-16 relative - the reference adds a row's K losses pairwise, the restatement
and the library in list order.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import dust_fixture
import dust_oracle
from conftest import ROOT


def test_oracle_reproduces_the_reference():
    f = dust_fixture.load()
    o = dust_fixture.oracle("count")
    assert f["amu"] == dust_oracle.AMU and f["critical_density"] == dust_oracle.CRITICAL_DENSITY
    fd, fr = f["ref_frac_destruction"], f["ref_frac_reuptake"]
    print("frac_reuptake worst |diff| / |ref| %.2e, / bound %.2e" % (
        dust_oracle.worst_ratio(o["frac_reuptake"], fr, np.abs(fr)),
        dust_oracle.worst_ratio(o["frac_reuptake"], fr, o["frac_reuptake_bound"])))
    assert np.array_equal(o["frac_destruction"], fd)
    dust_oracle.assert_within("frac_reuptake", o["frac_reuptake"], fr, o["frac_reuptake_bound"])
    # first-order bounds, not rtols: tight except on the few elements fed by a pair near the edge of a grain's support,
    # where s^2 - r^2 cancels
    for nm in dust_oracle.OUTPUTS:
        nz = o[nm] != 0.0
        rel = o[nm + "_bound"][nz] / np.abs(o[nm][nz])
        print(nm, "relative bound: median %.2e, worst %.2e" % (np.median(rel), rel.max()))
        assert np.median(rel) <= 1e-11, nm


def test_fixture_is_not_trivial():
    """Conditions on the inputs (a regenerated fixture that fails one changes its seed)."""
    f = dust_fixture.load()
    dusty = f["particle_type"] == 2
    fd, fr = f["ref_frac_destruction"], f["ref_frac_reuptake"]
    assert np.all(fd[~dusty] == 0.0) and np.any(fd[dusty] > 0.0) and np.all(fd >= 0.0)
    assert np.all(fr[f["particle_type"] != 0] == 0.0) and np.any(fr > 0.0)
    assert np.all(fd[:, :7] == 0.0) and np.all(fd[:, 13:] == 0.0) and np.all(np.any(fd[:, 7:13] > 0.0, axis=0))
    big = f["mass"][dusty] > f["crit_mass"]
    assert big.any() and not big.all()
    assert np.all(fd[dusty][~big] == 0.0)


@pytest.mark.parametrize("which", ["count", "fraction"])
def test_regimes_are_met(which):
    c = dust_fixture.oracle(which)["counts"]
    print(which, c, dust_fixture.oracle(which)["margins"])
    assert c["lost"] == c["accepted"] + c["rejected"] and c["rejected"] >= c["rejected_by_accumulation"]
    assert c["accepted"] > 0 and c["rejected"] > 0 and c["rejected_by_accumulation"] > 0
    assert (c["capped"] > 0) == (which == "fraction")


def test_fraction_guard_keeps_the_loss_below_the_atom_count():
    o = dust_fixture.oracle("fraction")
    assert np.all(o["frac_destruction"] < 1.0) and o["frac_destruction"].max() > 0.5
    assert dust_fixture.oracle("count")["frac_destruction"].max() < 1e-40


@pytest.mark.parametrize("name", list(dust_fixture.input_sets()))
def test_no_decision_within_reach_of_the_bound(name):
    """Every discrete decision of every input set the GPU tests use lies at least SLACK times the bound's relative size
    there away from its threshold: the library decides as the restatement does, its counts are equal, and the
    comparison leaves no element out."""
    if name.startswith("fixture"):
        o = dust_fixture.oracle("count" if name == "fixture" else "fraction")
    else:
        o = dust_fixture.run_oracle(dust_fixture.input_sets()[name]())
    print(name, o["counts"], "pairs", o["pairs"], "margins", o["margins"], "slack", o["slack"])
    for what, v in o["slack"].items():
        assert v >= dust_fixture.SLACK, (name, what, v, o["margins"][what])


def test_small_shapes_meet_the_regimes_between_them():
    tot = dict.fromkeys(dust_oracle.COUNTS, 0)
    for K in dust_fixture.CLOUD_K[1:]:
        for name, f in dust_fixture.shape_clouds(K):
            c = dust_fixture.run_oracle(f)["counts"]
            if f["points"].shape[0] > 200:
                assert c["accepted"] > 0, name
            for nm in tot:
                tot[nm] += c[nm]
    assert all(v > 0 for v in tot.values()), tot


@pytest.mark.parametrize("guard", ["count", "fraction"])
def test_hub_guard_flips_inside_the_slice(guard):
    f = dust_fixture.hub(guard)
    o = dust_fixture.run_oracle(f)
    c = o["counts"]
    assert o["pairs"] == 600 > 256 and c["accepted"] > 6 * 20 and c["rejected_by_accumulation"] > 6 * 20, c
    assert np.all(o["frac_destruction"][1:] == 0.0) and np.all(o["frac_destruction"][0, 7:13] > 0.0)


def test_missing_entries_contribute_nothing_and_empty_selectors_give_zeros():
    f = dust_fixture.short_cloud(5, 7)
    n = f["points"].shape[0]
    assert np.any(f["neighbor"] == n)
    o = dust_fixture.run_oracle(f)
    o2 = dust_fixture.run_oracle(dict(f, neighbor=f["neighbor"][:, :n]))
    for nm in dust_oracle.OUTPUTS:
        assert np.array_equal(o[nm], o2[nm]), nm
    assert o["pairs"] > 0 and o["counts"]["lost"] > 0
    g = dust_fixture.cloud(257, 7, 15, 5)
    z = dust_fixture.run_oracle(dict(g, species_curve=np.zeros(15, np.int32)))
    assert np.all(z["frac_destruction"] == 0.0) and np.all(z["frac_reuptake"] == 0.0) and z["counts"]["lost"] == 0
    assert dust_fixture.run_oracle(g)["counts"]["lost"] > 0


def test_a_repeated_index_counts_once_per_occurrence():
    f = dust_fixture.hub("count")
    nb = f["neighbor"].copy()
    nb[5] = [5, 0, 0]
    a = dust_fixture.run_oracle(dict(f, neighbor=nb))
    nb2 = nb.copy(); nb2[5] = [5, 0, 601]
    b = dust_fixture.run_oracle(dict(f, neighbor=nb2))
    assert a["pairs"] == b["pairs"] + 1
    assert a["frac_reuptake"][5, 7] > 1.5 * b["frac_reuptake"][5, 7] > 0.0


def test_default_selector_is_the_reference_s_tuple_padded():
    import sph_code_amd.compat as nsc
    assert tuple(nsc.dust_species_curve(15)) == (0, 0, 0, 0, 0, 0, 1, 2, 1, 2, 1, 1, 1, 0, 0)
    assert tuple(nsc.dust_species_curve(8)) == (0, 0, 0, 0, 0, 0, 1, 2) and tuple(nsc.dust_species_curve(32)[14:]) == (0,) * 18
    for S in (8, 15, 32):
        assert np.array_equal(nsc.dust_species_curve(S), dust_oracle.species_curve_default(S))
    with pytest.raises(ValueError):
        nsc.dust_species_curve(15, [0] * 14)
    with pytest.raises(ValueError):
        nsc.dust_species_curve(3, [0, 3, 0])
    assert (nsc.DUST_KNOTS_V, nsc.DUST_KNOTS_C, nsc.DUST_KNOTS_SI) == tuple(
        tuple(a) for a in (dust_oracle.KNOTS_V, dust_oracle.KNOTS_C, dust_oracle.KNOTS_SI))
    assert nsc.crit_mass == dust_oracle.CRIT_MASS and nsc.critical_density == dust_oracle.CRITICAL_DENSITY
    assert nsc.DUST_COUNTS == dust_oracle.COUNTS


def test_header_declares_and_library_exports_supernova_destruction():
    src = open(os.path.join(ROOT, "include", "sphx.h")).read()
    body = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for nm in ("sphx_supernova_destruction", "sphx_dust_last_timing"):
        assert re.search(r"\bint\s+%s\s*\(" % nm, body), nm
    for quirk in ("Q13", "NaN x False", "negative f_un", "d argument", "SPHX_DUST_GUARD_FRACTION", "once per occurrence"):
        assert quirk in src, quirk
    import sph_code_amd._lib as L
    lib = ctypes.CDLL(L.LIB_PATH)
    assert hasattr(lib, "sphx_supernova_destruction") and hasattr(lib, "sphx_dust_last_timing")
    assert len(L.SIGNATURES["sphx_supernova_destruction"][1]) == 23


def test_compat_signature_is_the_reference_s():
    import sph_code_amd.compat as nsc
    names = list(inspect.signature(nsc.supernova_destruction).parameters)
    assert names[:9] == ["points", "velocities", "neighbor", "mass", "f_un", "mu_array", "sizes", "densities",
                         "particle_type"]
    assert names[9:] == ["crit_mass", "critical_density", "species_curve", "guard", "full"]
    assert callable(nsc.dust_last_timing)
