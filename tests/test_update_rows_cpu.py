"""CPU side of the tests of the leapfrog/energy update's two classes of rows (sphx_update_rows.h): a stand-alone host
program replays the rules on random byte arrays - with and without sanitizers.  What the step does with them on the GPU:
tests/test_gpu_update_split.py."""
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
def test_a_row_is_settled_by_its_byte_alone(tmp_path, sanitize):
    """tests/host/update_rows_check.cpp, a check of sphx_update_loads_visc: a row takes the viscous sums as NaN exactly
    when its byte is not 0 (any non-zero byte is "settled"); a launch without bytes loads for every row."""
    cxx = _cxx()
    if cxx is None:
        pytest.skip("no host C++ compiler on this machine")
    exe = str(tmp_path / "update_rows_check")
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        ver = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
        if "clang" not in ver.lower():          # (GCC's runtimes, linked dynamically, insist on being loaded first)
            flags += ["-static-libasan", "-static-libubsan"]
    res = subprocess.run([cxx] + flags + ["-o", exe, os.path.join(ROOT, "tests", "host", "update_rows_check.cpp")],
                         capture_output=True, text=True)
    no_runtime = any(("cannot find" in ln or "no such file" in ln.lower()) and ("asan" in ln or "ubsan" in ln)
                     for ln in res.stderr.splitlines())
    if res.returncode != 0 and sanitize and no_runtime:
        pytest.skip("this compiler has no sanitizer runtimes: " + res.stderr.strip().splitlines()[-1])
    assert res.returncode == 0, res.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "sphx_update_rows: 0 violations" in run.stdout
    broken = [ln for ln in run.stdout.splitlines() if ln.startswith("broken rule:")]
    assert broken and int(broken[0].split()[2]) > 0              # the check can fail
