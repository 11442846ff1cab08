"""CPU tests of the dust phase's yardsticks (no GPU): tests/phase_oracle.py against what the reference driver's own
statements (code_running.py:399-435) leave behind (tests/golden/make_golden_phase.py), the conditions on the input sets
the GPU tests compare with an oracle, the one step the GPU tests take before the phase, and the slot arithmetic of the list
translation replayed on the host.  What the library does with all of it on the GPU: tests/test_gpu_phase.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import chem_oracle
import dust_oracle
import oracle_bounds as ob
import phase_fixture as pf
import phase_oracle as po
from conftest import ROOT
from oracle import sph_oracle as orc
from step_oracle import oracle_step

BOOK = ("mass_chem", "in_mu_array", "f_un_chem", "frac_destruction", "frac_reuptake")


def book_of(g, mu_key):
    return po.bookkeeping(g["mass_chem"], g[mu_key], g["f_un_chem"], g["frac_destruction"], g["frac_reuptake"], g["mu_specie"],
                          g["gamma"], float(g["crit_mass"]), mass_before=g.get("in_mass"))


def test_bookkeeping_reproduces_the_driver_on_stub_stages():
    """Case (b): stub stages with NaNs in both fraction arrays, NaN entries in f_un after chem, and losses that drive masses
    negative.  phase_oracle.bookkeeping gives the driver's mass, f_un, mu_array and gamma_array bit for bit (NumPy 1.26 on
    x86-64, 80-bit longdouble), the NaN fills and the resets at the same places, every reset mass negative by more than
    1e6 times its bound; the totals agree within their bounds (the driver's mass_reduction and mass_increase are float64
    sums over NaNs, hence NaN, as here)."""
    g = pf.load_golden("b")
    o = book_of(g, "in_mu_array")
    for name in po.BOOK_OUTPUTS:
        assert np.array_equal(o[name], g[name]), (name, dust_oracle.worst_ratio(o[name], g[name], o[name + "_bound"]))
    assert len(o["reset"]) > 10 and np.array_equal(o["reset"], np.nonzero(g["mass"] == g["crit_mass"] / 200.)[0])
    assert np.array_equal(o["filled"], np.argwhere(np.isnan(g["f_un_chem"] + np.nan_to_num(g["frac_reuptake"] - g["frac_destruction"]))))
    assert len(o["filled"]) > 10 and np.isnan(g["frac_destruction"]).any() and np.isnan(g["frac_reuptake"]).any()
    assert o["reset_margin"] >= 1e6, o["reset_margin"]
    for a, name in enumerate(po.TOTALS):
        ref, got = float(g["totals"][a]), o["totals"][name]
        assert (np.isnan(ref) and np.isnan(got)) or abs(got - ref) <= o["totals_bound"][name], (name, got, ref)


def test_chain_reproduces_the_driver_stage_by_stage():
    """Case (a): the reference's own stages on the sphere.  Each stage of phase_oracle.chain is fed the reference's
    previous outputs and held to that stage's existing bound: the density to oracle_bounds' for a positive loop sum,
    chemisputtering to chem_oracle's, sputtering to dust_oracle's (the reference's guard rejects every loss here: zeros
    on both sides), the bookkeeping to phase_oracle's."""
    f, g = pf.sphere(), pf.load_golden("a")
    given = {k_: g[k_] for k_ in ("density", "mass_chem", "f_un_chem", "frac_destruction", "frac_reuptake")}
    ch = po.chain(f["points"], f["velocities"], f["neighbor"], f["mass"], f["f_un"], f["mu_array"], f["sizes"], f["T"],
                  f["particle_type"], f["d"], f["dt"], f["crit_mass"], guard="count", mu_specie=f["mu_specie"], gamma=g["gamma"],
                  given=given, model=False)
    ob.pos_close(ch["density"], g["density"], "density", rtol=ob.RTOL_LOOP_POS)
    chem_oracle.assert_within("mass_new", ch["chem"]["mass_new"], g["mass_chem"], ch["chem"]["mass_new_bound"], "chem")
    chem_oracle.assert_within("f_un_new", ch["chem"]["f_un_new"], g["f_un_chem"], ch["chem"]["f_un_new_bound"], "chem")
    assert ch["dust"]["counts"]["lost"] > 0 and ch["dust"]["counts"]["accepted"] == 0
    for name in dust_oracle.OUTPUTS:
        dust_oracle.assert_within(name, ch["dust"][name], g[name], ch["dust"][name + "_bound"], "dust")
    for name in po.BOOK_OUTPUTS:
        dust_oracle.assert_within(name, ch["book"][name], g[name], ch["book"][name + "_bound"], "bookkeeping")
    moved = np.count_nonzero(np.abs(g["mass"] - f["mass"]) > 1e-6 * f["mass"])
    assert moved >= 1000, moved


def test_sphere_set_meets_the_conditions():
    """The set the GPU tests compare with an oracle, under guard="fraction": contributing rows, at least three rounds,
    accepted losses, both stages' slacks >= 1e6, at least 1000 masses moved by more than 1e-6."""
    f = pf.sphere()
    ch = po.chain(f["points"], f["velocities"], f["neighbor"], f["mass"], f["f_un"], f["mu_array"], f["sizes"], f["T"],
                  f["particle_type"], f["d"], f["dt"], f["crit_mass"], guard="fraction", mu_specie=f["mu_specie"], gamma=f["gamma"])
    fig = po.conditions(ch, f["mass"])
    print(fig, ch["chem"]["counts"], ch["dust"]["counts"])
    assert ch["book"]["reset_margin"] >= 1e6


SETS = [("sphere", None)] + [(pf.shape_id(s), s) for s in pf.SHAPES]


@pytest.mark.parametrize("name,spec", SETS, ids=[s[0] for s in SETS])
def test_the_one_step_moves_nothing_further_than_a_hundredth_of_h(name, spec):
    """The fixed step of every set, taken by the oracle in both step modes: finite, and no particle moves further than
    1 % of its h - the list the phase then runs on is one update older than the points, as in the driver, and barely so."""
    f = pf.sphere() if spec is None else pf.state(*spec)
    s0 = pf.sim_state(f)
    n = len(f["mass"])
    K = f["neighbor"].shape[1]
    for forms in ("loop", "hydro_update"):
        with np.errstate(all="ignore"):
            s1 = oracle_step((forms, "cloud", n, K), s0, f["d"], True, f["fixed_dt"])
        move = np.sqrt(np.sum((s1["points"] - s0["points"]) ** 2, axis=1))
        assert np.isfinite(s1["points"]).all() and np.isfinite(s1["T"]).all()
        assert np.max(move / s1["sizes"]) <= pf.MOVE_LIMIT, (forms, np.max(move / s1["sizes"]))
        assert move.max() > 0


@pytest.mark.parametrize("S", [7, 8, 15, 16, 17, 32])
def test_numpy_adds_a_row_as_the_drag_refresh_assumes(S):
    """The drag refresh of the phase adds table[t] * f_un[i, t] over t in the order np.sum(table * f_un, axis=1) does
    (phase_oracle.numpy_row_sum, phase_np_sum in sphx_phase.hip), so that the refreshed coefficients are the ones
    Simulation forms at upload.  Here: that order is the installed NumPy's, on rows whose sum depends on it."""
    rs = np.random.RandomState(S)
    a = rs.uniform(0.0, 1.0, (4096, S)) * 10.0 ** rs.uniform(-8, 8, (4096, S))
    assert np.array_equal(po.numpy_row_sum(a), np.sum(a, axis=1))
    assert S < 8 or not np.array_equal(np.cumsum(a, axis=1)[:, -1], np.sum(a, axis=1))      # (the order matters)


def _cxx():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


def _host_check(tmp_path, name, sanitize, verdict):
    """Builds tests/host/<name>.cpp (with sanitizers: a program of its own) and runs it: it must report `verdict`, and a
    deliberately broken rule must fail inside it (the program prints how often)."""
    cxx = _cxx()
    if cxx is None:
        pytest.skip("no host C++ compiler on this machine")
    exe = str(tmp_path / name)
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        ver = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
        if "clang" not in ver.lower():
            flags += ["-static-libasan", "-static-libubsan"]
    res = subprocess.run([cxx] + flags + ["-o", exe, os.path.join(ROOT, "tests", "host", name + ".cpp")],
                         capture_output=True, text=True)
    no_runtime = any(("cannot find" in ln or "no such file" in ln.lower()) and ("asan" in ln or "ubsan" in ln)
                     for ln in res.stderr.splitlines())
    if res.returncode != 0 and sanitize and no_runtime:
        pytest.skip("this compiler has no sanitizer runtimes: " + res.stderr.strip().splitlines()[-1])
    assert res.returncode == 0, res.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert verdict in run.stdout
    broken = [ln for ln in run.stdout.splitlines() if ln.startswith("broken rule:")]
    assert broken and int(broken[0].split()[2]) > 0              # the check can fail


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_list_translation_slot_arithmetic_on_the_host(tmp_path, sanitize):
    """tests/host/phase_map_check.cpp replays sphx_phase_map.h's two passes over random storage orders, processing orders
    and lists with missing entries (n = 1, 33, 63 .. 65, 257, 2049; K = 1, 7, 40, 64) against a direct construction, and
    the (n,k) int64 form; a rule that forgets the processing order must break it (the program fails otherwise)."""
    _host_check(tmp_path, "phase_map_check", sanitize, "sphx_phase_map: 0 violations")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_reverse_list_size_rules_on_the_host(tmp_path, sanitize):
    """tests/host/revlist_check.cpp checks sphx_revlist.h, the size rules of the reverse list that rad_cooling,
    supernova_destruction and chemisputtering_2 build with sphx_rev_build, by brute force: the sort looks at the least b in
    [1, 32] bits with 2^b >= key_end (key_end = 1 .. 5, 2^16 - 1 .. 2^16 + 1, 2^31 - 16), and for M = 0, 1, 3, 4, 5, 1023
    the sorted half starts on a 16-byte boundary at least M ints behind the raw one and both fit the ints ensured."""
    _host_check(tmp_path, "revlist_check", sanitize, "sphx_revlist: 0 violations")
