"""CPU tests of the radiative phase's yardsticks (no GPU): tests/radphase_oracle.py against what the reference driver's own
statements (code_running.py:247-316) and rad_heating's frame leave behind (tests/golden/make_golden_radphase.py), the
host-side setup of compat (rad_setup, stellar_spectrum, luminosity_relation) against the reference's captured selection
and spectrum, and the per-particle formulas of sphx_radphase_pair.h replayed on the host.  What the library does with
them on the GPU: tests/test_gpu_radphase.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import rad_fixture
import radphase_fixture as rf
import radphase_oracle as ro
import sph_code_amd.compat as nsc
from conftest import ROOT

CASES = [("a", "ionise"), ("a", "heat"), ("a", "cool"), ("b", "heat"), ("b", "cool")]


@pytest.mark.parametrize("case,stage", CASES, ids=["%s-%s" % c for c in CASES])
def test_oracle_reproduces_the_driver_stage_by_stage(case, stage):
    """Each stage of the restatement, fed the reference's own previous outputs, meets what the reference left within the
    restatement's own bound, element by element; case (b) covers E_internal = 0, negative E_internal, NaN lf2, both
    clamps and an underflowing exp.  The clamp counts are those the reference's results show."""
    o, ref = rf.oracle(case, stage), rf.reference(case, stage)
    for name, want in ref.items():
        w = ro.assert_within(name, o[name], want, o[name + "_bound"], "%s/%s" % (case, stage))
        print("%s/%s %-14s worst |difference| / bound = %.3g" % (case, stage, name, w))
    if stage != "ionise":
        g = rf.load(case)
        T, T_in = ref["T"], g["T"] if stage == "heat" else g["heat_T"]
        # T < t_cmb is strict: a star's T, which is not formed anew, does not count again when an earlier clamp left it at
        # t_cmb; T >= t_max is not: every entry at t_max counts
        kept = np.count_nonzero((g["particle_type"] == 1) & (T_in == float(g["const_t_cmb"])))
        lo, hi = o["counts"]["T_raised"]
        assert lo <= np.count_nonzero(T == float(g["const_t_cmb"])) - kept <= hi
        lo, hi = o["counts"]["T_lowered"]
        assert lo <= np.count_nonzero(T == float(g["t_max"])) <= hi
        assert min(o["counts"]["T_raised"][0], o["counts"]["T_lowered"][0], o["counts"]["E_raised"][0]) > 0


def test_fixture_b_holds_every_regime():
    g = rf.load("b")
    pt = g["particle_type"]
    gas_lf2 = g["rh_lf2"][pt[pt != 1] == 0]
    E = g["E_internal"][pt == 0]
    assert np.any(E == 0) and np.any(E < 0) and np.isnan(gas_lf2).any() and np.any(gas_lf2 == 0)
    assert np.any((E == 0) & (gas_lf2 > 0))                      # inf -> DBL_MAX
    with np.errstate(all="ignore"):
        n_part = g["mass"] / (float(g["const_m_h"]) * g["end_mu_array"])
        c1 = -(g["cool_energy"] * n_part)[pt == 0] / g["heat_E_internal"][pt == 0]
    assert np.any(c1 < -746) and np.any(c1 > 0)                   # the exp underflows; the + 1 branch
    assert np.any(pt == 2) and np.any(pt == 1)


@pytest.mark.parametrize("case", rad_fixture.CASES)
def test_rad_setup_reproduces_the_reference_selection(case):
    """With the global np.random seeded as make_golden_rad.py seeded it, compat.rad_setup picks the reference's stars and
    gas particles and gives its luminosities: rs2, rg2 and luminosities bit for bit."""
    seed = {"sphere_dust_n2048_k40": 5101, "condensed_n1024_k40": 5102}[case]
    f = rad_fixture.load(case)
    np.random.seed(seed)
    src, lum, dst = nsc.rad_setup(f["ptypes"], f["masses"], np.zeros(0, np.int64), f["dt"])
    assert np.array_equal(f["positions"][src], f["sources"])
    assert np.array_equal(f["positions"][dst], f["targets"])
    assert np.array_equal(lum, f["luminosities"])
    assert np.all(f["ptypes"][src] == 1) and np.all(f["ptypes"][dst] != 1)


def test_rad_setup_quirks():
    """None drawn -> all stars; a supernova adds its term before the renormalisation; the total is that of all stars; no
    star -> no source and every non-star particle a target."""
    class Fixed(object):
        def __init__(self, *vals):
            self.vals = list(vals)

        def rand(self, n):
            return np.full(n, self.vals.pop(0))
    pt = np.array([0, 1, 2, 1, 0, 0, 1.0])
    m = np.array([1, 0.5, 1, 2.0, 1, 1, 1.0]) * nsc.solar_mass
    light = np.where(pt == 1, 0.5 * nsc.solar_mass, m)              # 0.5 / 4 + 3^-0.5 = 0.702 < 0.999: none drawn
    src, lum, dst = nsc.rad_setup(pt, light, [], 1e12, rng=Fixed(0.999, 0.999))
    assert src.tolist() == [1, 3, 6] and dst.tolist() == []
    assert abs(np.sum(lum) - 3 * 0.35 * 0.5 ** 2.62) <= 1e-15
    total = np.sum(nsc.luminosity_relation(m[pt == 1] / nsc.solar_mass))
    src2, lum2, dst2 = nsc.rad_setup(pt, m, [3], 1e12, rng=Fixed(0.75, 0.0))
    assert src2.tolist() == [3, 6] and dst2.tolist() == [0, 2, 4, 5]  # m / 4 + 3^-0.5 = 0.702, 1.077, 0.827 against 0.75
    base = nsc.luminosity_relation([2.0, 1.0]) + np.array([0.264 * nsc.supernova_energy / nsc.solar_luminosity / 1e12, 0.0])
    assert np.array_equal(lum2, base / np.sum(base) * total)
    src3, lum3, dst3 = nsc.rad_setup(np.array([0, 2, 0.0]), m[:3], [], 1e12, rng=Fixed(0.9))
    assert len(src3) == 0 and len(lum3) == 0 and dst3.tolist() == [0, 1, 2]


def test_stellar_spectrum_reproduces_the_captured_spectrum():
    """frac_dest and n_photons = photons_per_joule lf2 as rad_heating's frame held them (case (a)), bit for bit; so are
    the tables and constants the defaults of the array calls come from."""
    g = rf.load("a")
    frac, ppj = nsc.stellar_spectrum(g["mass"][g["particle_type"] == 1])
    assert np.array_equal(frac, g["rh_frac_dest"])
    assert np.array_equal(ppj * g["rh_lf2"], g["rh_n_photons"])
    assert np.array_equal(nsc.cross_sections, g["nsc_cross_sections"])
    assert np.array_equal(nsc.driver_cross_sections(), g["driver_cross_sections"])
    assert np.array_equal(nsc.destruction_energies, g["destruction_energies"])
    for name in ("k", "m_h", "amu", "sb", "t_cmb"):
        assert getattr(nsc, name) == float(g["const_" + name]), name


def test_luminosity_relation_on_both_sides_of_its_breaks():
    """The luminosity law breaks at 0.7 solar masses, the lifetime is floored at 3.6e-4; the radius law's break at 1.66
    does not show in either (it feeds the spectrum's temperature)."""
    lo, hi = np.nextafter(0.7, 0), 0.7
    lum = nsc.luminosity_relation(np.array([lo, hi, 1.0, np.nextafter(1.66, 0), 1.66, 40.0]))
    assert lum[0] == 0.35 * lo ** 2.62 and lum[1] == 1.02 * hi ** 3.92 and lum[2] == 1.02
    assert lum[3] == 1.02 * np.nextafter(1.66, 0) ** 3.92 and lum[4] == 1.02 * 1.66 ** 3.92
    life = nsc.luminosity_relation(np.array([lo, hi, 1.0, 14.0, 16.0, 100.0]), 1)
    assert life[0] == 0.35 ** -1 * lo ** (1 - 2.62) and life[1] == 1.02 ** -1 * hi ** (1 - 3.92) and life[2] == 1.02 ** -1
    assert life[3] == 1.02 ** -1 * 14.0 ** (1 - 3.92) > 3.6e-4       # the floor is met at 15.0 solar masses
    assert life[4] == 3.6e-4 and life[5] == 3.6e-4
    assert nsc.luminosity_relation(np.array([np.nan]))[0] == 0.0     # neither side of the break: the reference's zeros


def _cxx():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_pair_formulas_on_the_host(tmp_path, sanitize):
    """tests/host/radphase_check.cpp compiles sphx_radphase_pair.h for the host and replays every regime of case (b) on
    rows of 6 .. 32 species against the formulas in long double; a rule that forgets nan_to_num must break it."""
    cxx = _cxx()
    if cxx is None:
        pytest.skip("no host C++ compiler on this machine")
    exe = str(tmp_path / "radphase_check")
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        ver = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
        if "clang" not in ver.lower():
            flags += ["-static-libasan", "-static-libubsan"]
    res = subprocess.run([cxx] + flags + ["-o", exe, os.path.join(ROOT, "tests", "host", "radphase_check.cpp")],
                         capture_output=True, text=True)
    no_runtime = any(("cannot find" in ln or "no such file" in ln.lower()) and ("asan" in ln or "ubsan" in ln)
                     for ln in res.stderr.splitlines())
    if res.returncode != 0 and sanitize and no_runtime:
        pytest.skip("this compiler has no sanitizer runtimes: " + res.stderr.strip().splitlines()[-1])
    assert res.returncode == 0, res.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "sphx_radphase_pair: 0 violations" in run.stdout
    broken = [ln for ln in run.stdout.splitlines() if ln.startswith("broken rule:")]
    assert broken and int(broken[0].split()[2]) > 0              # the check can fail
