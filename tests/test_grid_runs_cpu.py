"""CPU check of the rule the fused cell count aggregates its histogram atomics by (sphx_run_of_lane, sphx_runs.h: head
mask -> run length, base, arrival number), replayed by a stand-alone host program over random and adversarial waves of
cell ids, partial waves included - with and without sanitizers.  What the kernel does with it on the GPU:
tests/test_gpu_grid_count_runs.py."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def _cxx():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_run_rule_hands_every_cell_a_permutation(tmp_path, sanitize):
    """tests/host/grid_runs_check.cpp: one cell for all, one cell each, A B A B, pairs cut by a wave's end, random sorted
    runs, unsorted cells; n = 1, 63 .. 65, 127 .. 129, 193, 300, 700, 1000 and random.  The histogram must equal the plain
    count, every cell's arrival numbers must be a permutation of 0 .. count - 1 ascending inside a run, with one atomic
    add per run; a rule that ignores the end of the active lanes must break that (the program fails otherwise)."""
    cxx = _cxx()
    if cxx is None:
        pytest.skip("no host C++ compiler on this machine")
    exe = str(tmp_path / "grid_runs_check")
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        # (GCC links the sanitizer runtimes dynamically by default, and they then insist on being the first library the
        #  process loads; linked into the program itself they do not care what else the environment loads)
        ver = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
        if "clang" not in ver.lower():
            flags += ["-static-libasan", "-static-libubsan"]
    res = subprocess.run([cxx] + flags + ["-o", exe, os.path.join(ROOT, "tests", "host", "grid_runs_check.cpp")],
                         capture_output=True, text=True)
    # (only the linker not finding the runtimes is a reason to skip: any other failure under -fsanitize is a failure)
    no_runtime = any(("cannot find" in ln or "no such file" in ln.lower()) and ("asan" in ln or "ubsan" in ln)
                     for ln in res.stderr.splitlines())
    if res.returncode != 0 and sanitize and no_runtime:
        pytest.skip("this compiler has no sanitizer runtimes: " + res.stderr.strip().splitlines()[-1])
    assert res.returncode == 0, res.stderr
    run = subprocess.run([exe, "2000"], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    out = run.stdout
    assert "sphx_run_of_lane: 0 violations" in out
    broken = [ln for ln in out.splitlines() if ln.startswith("broken rule:")]
    assert broken and int(broken[0].split()[2]) > 0              # the check can fail
