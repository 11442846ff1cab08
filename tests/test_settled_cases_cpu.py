"""CPU side of the tests of the sums that are NaN before they are finished (sphx_settled.h): the oracle shows that no
case of tests/settled_cases.py is vacuous, and a stand-alone host program replays the two rules - with and without
sanitizers.  What the LDS passes do with them on the GPU: tests/test_gpu_settled_sums.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import settled_cases as sc
from conftest import ROOT
from oracle import sph_oracle as orc


def _oracle(state, K):
    idx, h = sc.knn(state["points"], K)
    with np.errstate(all="ignore"):
        out, inter = orc.hydro_update(*sc.hydro_args_of(state, idx, h), return_intermediates=True)
    Pi = np.sum(inter["pi"], axis=1)
    Bw = state["mass"] * Pi * (state["particle_type"] == 0.)
    return idx, out, inter["pi"], Bw


@pytest.mark.parametrize("K", sc.KS)
@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_no_case_is_vacuous(variant, K):
    st, bad = sc.make_case(variant, K)
    idx, out, pi, Bw = _oracle(st, K)
    va, vh = out[1], out[2]
    n = len(va)
    assert n == 3 * sc.N_CLUMP and idx.shape == (n, K)
    # no list crosses between the clumps, and every list is full
    clump = np.arange(n) // sc.N_CLUMP
    assert (idx < n).all() and (clump[idx] == clump[:, None]).all()
    assert (idx[:, 0] == np.arange(n)).all()                              # rank 0: the particle itself
    nan_row = np.isnan(va).any(axis=1)
    assert (np.isnan(va).all(axis=1) == nan_row).all() and (np.isnan(vh) == nan_row).all()
    assert not np.isinf(va).any() and not np.isinf(vh).any()
    assert nan_row[sc.A].all() and np.isnan(Bw[sc.A]).all()               # A: all NaN, every row settled
    assert not nan_row[sc.B].any() and np.isfinite(Bw[sc.B]).all()        # B: all finite
    assert nan_row[sc.C].any() and not nan_row[sc.C].all()                # C: both
    own_nan = np.isnan(Bw)
    assert (st["T"][sc.C] < 0).sum() == 1 and st["T"][bad] < 0
    lists_bad = (idx == bad).any(axis=1)
    if variant == "self":
        assert lists_bad.sum() == 1 and lists_bad[bad]                    # the rank-0 entry of its own list, nothing else
        assert nan_row[sc.C].sum() == 1 and nan_row[bad] and own_nan[sc.C].sum() == 1
    else:
        # rows whose own m Pi is finite but whose viscous sums are NaN (a neighbour's m Pi is)
        assert (nan_row[sc.C] & ~own_nan[sc.C]).any()
        assert (own_nan[sc.C] == lists_bad[sc.C]).all()                   # Pi is NaN exactly where the bad one is listed
        # mixed waves: among 16 consecutive rows of C both kinds (whatever order the blobs take them in, C is mixed)
        assert 0 < own_nan[sc.C].sum() < sc.N_CLUMP
    if variant == "last":
        rows = np.nonzero(idx[:, K - 1] == bad)[0]
        assert len(rows) > 0
        # ... and for those rows it is the only NaN term: the sum is finite until the last list position
        assert np.isfinite(pi[rows, :K - 1]).all() and np.isnan(pi[rows, K - 1]).all()
    if variant == "dust":
        dust = st["particle_type"] == 2.
        assert dust[sc.A].sum() > 50 and dust[sc.C].sum() > 50 and not dust[sc.B].any()
        assert nan_row[sc.A][dust[sc.A]].all()                            # dust rows are settled too: 0 x NaN
        assert (nan_row[sc.C] & dust[sc.C]).any() and (~nan_row[sc.C] & dust[sc.C]).any()


def test_healthy_clump_alone_is_finite():
    st, bad = sc.make_case("centre", 40, clumps="B")
    assert bad is None and len(st["points"]) == sc.N_CLUMP
    _, out, _, Bw = _oracle(st, 40)
    assert np.isfinite(out[1]).all() and np.isfinite(out[2]).all() and np.isfinite(Bw).all()


def _cxx():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_settled_rules_on_every_class_of_double(tmp_path, sanitize):
    """tests/host/settled_check.cpp: NaN of either sign and any payload settles a row (given a first list position and
    an output to write), +-inf, +-0, denormal and finite values do not; NaN x anything is NaN; the quad's OR equals
    "the total (p0 + p1) + (p2 + p3) is NaN" for all 16 NaN patterns of four partials; a NaN partial stays NaN; the rule
    on a wave's lane masks (sphx_wave_saturated) equals "every row that sums is saturated" for every pattern in every
    row and for random waves with rows that do not sum."""
    cxx = _cxx()
    if cxx is None:
        pytest.skip("no host C++ compiler on this machine")
    exe = str(tmp_path / "settled_check")
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        ver = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
        if "clang" not in ver.lower():          # (GCC's runtimes, linked dynamically, insist on being loaded first)
            flags += ["-static-libasan", "-static-libubsan"]
    res = subprocess.run([cxx] + flags + ["-o", exe, os.path.join(ROOT, "tests", "host", "settled_check.cpp")],
                         capture_output=True, text=True)
    no_runtime = any(("cannot find" in ln or "no such file" in ln.lower()) and ("asan" in ln or "ubsan" in ln)
                     for ln in res.stderr.splitlines())
    if res.returncode != 0 and sanitize and no_runtime:
        pytest.skip("this compiler has no sanitizer runtimes: " + res.stderr.strip().splitlines()[-1])
    assert res.returncode == 0, res.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "sphx_settled: 0 violations" in run.stdout
    broken = [ln for ln in run.stdout.splitlines() if ln.startswith("broken rule:")]
    assert broken and int(broken[0].split()[2]) > 0              # the check can fail
