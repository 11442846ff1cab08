"""CPU side of the census' tests: the NumPy restatement (tests/census_oracle.py) against the fixtures the reference driver's
own statements left (tests/golden/census_a.npz, census_b.npz; make_golden_census.py), and a stand-alone host program that
replays the kernel's term arithmetic and LDS places (tests/host/census_check.cpp) - with and without sanitizers.  What the
library does with them on the GPU: tests/test_gpu_census.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import census_oracle as co
import sn_oracle
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = ("census_a", "census_b")
_cache = {}


def fixture(name):
    if name not in _cache:
        _cache[name] = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    return _cache[name]


def species_bounds(g):
    """The derived bound of every by-species sum of a fixture: 2 n_t 2^-53 sum|term| over the n_t rows of its mask."""
    S = g["f_un"].shape[1]
    t = co.terms(g["mass"], g["particle_type"], g["f_un"], g["mu_specie"])
    out = {}
    for ty, nm in enumerate(("gas_mass_by_species", "star_mass_by_species", "dust_mass_by_species")):
        n_t = int(np.count_nonzero(g["particle_type"] == ty))
        out[nm] = np.array([co.sum_bound(t[co.FIXED + ty * S + q], n_t) for q in range(S)])
    return out


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def test_the_many_quantity_order_is_the_ordered_total():
    """census_oracle.ordered_totals is sn_oracle.ordered_total for every row, also across the chunk and lane edges."""
    rng = np.random.RandomState(5)
    for n in (1, 255, 256, 257, 513, 65793):
        v = rng.normal(size=(2, n)) * np.exp(rng.normal(size=(2, n)) * 3)
        got = co.ordered_totals(v)
        for q in range(2):
            assert bits(got[q]) == bits(sn_oracle.ordered_total(v[q])), (n, q)


@pytest.mark.parametrize("name", CASES)
def test_restatement_against_the_driver_exact_items(name):
    g = fixture(name)
    m, pt, f, ages = g["mass"], g["particle_type"], g["f_un"], g["star_ages"]
    pos, max_rel, _ = co.schedule(ages, pt, m)
    assert np.array_equal(pos, g["out_supernova_pos"])
    assert bits(max_rel) == bits(g["out_max_rel_age"])
    # restricted to the star rows, as the library evaluates it
    stars = co.select(pt, 1)
    pos_s, max_rel_s, _ = co.schedule(ages[stars], pt[stars], m[stars])
    assert np.array_equal(stars[pos_s], g["out_supernova_pos"]) and bits(max_rel_s) == bits(g["out_max_rel_age"])
    after = co.advance(ages, pt, float(g["dt"]))
    assert np.array_equal(bits(after), bits(g["out_star_ages"]))
    assert np.array_equal(bits(g["T"][co.select(pt, 2)]), bits(g["out_dust_temps"]))
    agb = co.agb_outputs(m, pt, f, after, float(g["OVERALL_AGE"]), g["mu_specie"])
    assert np.array_equal(agb["AGB_condition"], g["out_AGB_condition"])
    assert np.array_equal(co.select(pt, 1, m, (1., 7.)), np.flatnonzero(g["out_AGB_condition"]))
    for k in ("AGB_list", "AGB_time_until", "AGB_metallicity", "AGB_composition"):
        assert np.array_equal(bits(agb[k]), bits(g["out_" + k])), k
    cen = co.census(m, pt, f, g["mu_specie"])
    assert cen["n_dust"] == g["out_dust_temps"].shape[0]
    assert bits(cen["star_numfrac"]) == bits(g["out_star_numfrac"])


@pytest.mark.parametrize("name", CASES)
def test_restatement_against_the_driver_sums(name):
    g = fixture(name)
    m, pt = g["mass"], g["particle_type"]
    cen = co.census(m, pt, g["f_un"], g["mu_specie"])
    bounds = species_bounds(g)
    worst = 0.0
    for nm, b in bounds.items():
        ref = g["out_" + nm]
        if not np.any(pt == ("gas_mass_by_species", "star_mass_by_species", "dust_mass_by_species").index(nm)):
            assert np.all(ref == 0) and np.all(cen[nm] == 0)             # np.sum over no row
            continue
        err = np.abs(cen[nm] - ref)
        worst = max(worst, float(np.max(err / b)))
        assert np.all(err <= b), (nm, err, b)
    print("worst |got - ref| / bound:", worst)
    # star_massfrac through the bounds of its two sums: |d(a/b)| <= (da + |a/b| db) / (|b| - db)
    a_ref, b_ref = float(np.sum(m[pt == 1])), float(np.sum(m[pt != 2]))
    da = co.sum_bound(m[pt == 1], int(np.count_nonzero(pt == 1)))
    db = co.sum_bound(m[pt != 2], int(np.count_nonzero(pt != 2)))
    assert abs(cen["star_mass"] - a_ref) <= da and abs(cen["nondust_mass"] - b_ref) <= db
    frac = float(g["out_star_massfrac"])
    assert abs(cen["star_massfrac"] - frac) <= (da + abs(frac) * db) / (abs(b_ref) - db) + 2.0 ** -52 * abs(frac)


def test_masked_rows_do_not_reach_the_other_types():
    """A NaN mass, a NaN composition and a zero row sum in dust rows: the gas and star quantities keep their bits."""
    s = co.make_state(11, 700, 15)
    clean = co.census(**{k: s[k] for k in ("mass", "particle_type", "f_un", "mu_specie")})
    dust = np.flatnonzero(s["particle_type"] == 2)
    m, f = s["mass"].copy(), s["f_un"].copy()
    m[dust[0]] = np.nan; f[dust[1], 3] = np.nan; f[dust[2]] = 0.0
    got = co.census(m, s["particle_type"], f, s["mu_specie"])
    for k in ("gas_mass", "star_mass", "gas_mass_by_species", "star_mass_by_species"):
        assert np.array_equal(bits(got[k]), bits(clean[k])), k
    assert np.isnan(got["dust_mass"]) and np.all(np.isnan(got["dust_mass_by_species"]))


def _cxx():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_term_arithmetic_and_tile_places_on_the_host(tmp_path, sanitize):
    """tests/host/census_check.cpp: the kernel's tile loop replayed with sphx_census_terms.h gives the left-to-right sum of
    every quantity, no two entries share a place of the tile, the row sum is NumPy's, masked rows give +0.0."""
    cxx = _cxx()
    if cxx is None:
        pytest.skip("no host C++ compiler on this machine")
    exe = str(tmp_path / "census_check")
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        ver = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
        if "clang" not in ver.lower():          # (GCC's runtimes, linked dynamically, insist on being loaded first)
            flags += ["-static-libasan", "-static-libubsan"]
    res = subprocess.run([cxx] + flags + ["-o", exe, os.path.join(ROOT, "tests", "host", "census_check.cpp")],
                         capture_output=True, text=True)
    no_runtime = any(("cannot find" in ln or "no such file" in ln.lower()) and ("asan" in ln or "ubsan" in ln)
                     for ln in res.stderr.splitlines())
    if res.returncode != 0 and sanitize and no_runtime:
        pytest.skip("this compiler has no sanitizer runtimes: " + res.stderr.strip().splitlines()[-1])
    assert res.returncode == 0, res.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "sphx_census: 0 violations" in run.stdout
    broken = [ln for ln in run.stdout.splitlines() if ln.startswith("broken rule:")]
    assert broken and int(broken[0].split()[2]) > 0              # the check can fail
