"""CPU side of the projected maps' tests: the NumPy restatement (tests/map_oracle.py) anchored to the samplers' restatement
(tests/arb_oracle.py, itself pinned to the reference's golden outputs), its quadrature, the absence of edge pairs in every
input the GPU tests use (tests/map_cases.py), and a stand-alone host program that replays the tile walk with
sphx_map_pair.h (tests/host/map_check.cpp) - with and without sanitizers.  What the library does with them on the GPU:
tests/test_gpu_map.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import arb_oracle as ao
import map_cases as mc
import map_oracle as mo
from conftest import ROOT


def test_the_closed_form_is_the_reference_kernel_integrated():
    """For random (R, b, m): the term c s^3 sqrt(s) equals the 4-point Gauss-Legendre quadrature over the chord
    [-sqrt(s), sqrt(s)] of Weigh2 (gas, R = h(m)) and of Weigh2_dust (dust, R = sizes) as arb_oracle.fields states them - the
    integrand is a polynomial of degree 6 in z, so four points are exact.  64 * 2^-53 relative: the roundings of the four
    terms and of the power.  b <= R / 2 keeps 1 - r^2 / R^2 away from the cancellation at the support's edge, which would
    amplify the quadrature's own roundings, not the closed form's."""
    rng = np.random.RandomState(7)
    x, w = np.polynomial.legendre.leggauss(4)
    d, m_0 = 3.0e17, mc.M_0
    worst = 0.0
    for trial in range(400):
        dust = trial % 2 == 1
        m = m_0 * rng.uniform(0.05, 3.0)
        R = float(rng.uniform(0.2, 2.0) * 1e17) if dust else float(np.cbrt(m / m_0) * d)
        b = R * rng.uniform(0.0, 0.5)
        s = R * R - b * b
        half = np.sqrt(s)
        q = np.stack((np.full(4, b), np.zeros(4), half * x), axis=1)             # the four points of the chord
        # two members per ball (the samplers return 0 for a ball of one): the particle and a star, which weighs nothing
        pts = np.zeros((2, 3))
        rs, mem = ao.to_csr([[0, 1]] * 4)
        out = ao.fields(pts, np.array([m, m]), np.array([2.0 if dust else 0.0, 1.0]), np.array([R, R]), np.array([10.0, 10.0]), None, None,
                        d, m_0, q, rs, mem)
        W = out["dust_density" if dust else "density"]
        quad = half * float(np.sum(w * W))
        closed = float(mo.term(mo.coeff(m, R), s))
        rel = abs(closed - quad) / abs(quad)
        worst = max(worst, rel)
        assert rel <= 64 * 2.0 ** -53, (trial, dust, rel / 2.0 ** -53)
    print("worst |closed - quadrature| / |quadrature| = %.3g ulp(2^-53)" % (worst / 2.0 ** -53))
    assert abs(mo.C_MAP - (32.0 / 35.0) * ao.C_W6) <= 2.0 ** -52 * mo.C_MAP


def test_the_columns_integrate_to_the_mass():
    """Sum of gas_column times the pixel area tends to the gas mass whose footprints lie in the window as pixels shrink: a
    check of the restatement alone, at a loose tolerance.  The gas footprints of this fixture are a good part of the window
    wide (h(m) at loop_d), many pixels even at 33 x 65, where the midpoint rule on such a smooth bump is far better than
    1e-3; it must fall as the pixels shrink."""
    s = mc.fixture("sphere_dust_n2048_k40")
    gas = s["particle_type"] == 0
    R = np.cbrt(s["mass"] / mc.M_0) * s["d"]
    hw = float(np.max(np.abs(s["points"][gas][:, 1:])) + np.max(R[gas])) * 1.01       # every gas footprint inside
    mass = float(np.sum(s["mass"][gas]))
    errs = []
    for npix in ((33, 65), (66, 130)):
        r = mo.project(s["points"], s["mass"], s["particle_type"], s["sizes"], s["T"], s["d"], mc.M_0, half_width=(hw, hw), npix=npix)
        area = (2 * hw / npix[0]) * (2 * hw / npix[1])
        errs.append(abs(float(np.sum(r["gas_column"])) * area - mass) / mass)
    print("relative error of the integrated gas column at 33 x 65, 66 x 130:", errs)
    assert errs[0] <= 1e-3 and errs[1] <= 1e-4 and errs[1] < errs[0]


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_no_pair_on_an_edge_in_the_gpu_inputs(name):
    """edge == 0 (and no pixel centre on a bounding box's side) on every input tests/test_gpu_map.py uses: count, skipped
    and pairs may then be compared for equality although a gas radius may differ by an ulp between the two sides."""
    r = mc.reference(name)
    assert r["edge"] == 0 and r["box_edge"] == 0, (name, r["edge"], r["box_edge"])


def test_the_cases_cover_what_they_are_named_for():
    c, ref = mc.CASES, mc.reference
    assert ref("beside")["pairs"] == 0 and ref("all-stars")["pairs"] == 0 and ref("all-stars")["skipped"] == 0
    assert ref("bad-rows")["skipped"] == 6 and ref("bad-rows")["pairs"] > 0
    assert ref("zoom20")["count"].min() > 100
    half = ref("half-off")["count"]
    assert not half[:, half.shape[1] * 3 // 4:].any() and half[:, :half.shape[1] // 4].any()
    assert ref("between-centres")["count"].sum() == 1 and ref("between-centres")["pairs"] == 2
    k = c["on-a-centre"]
    p = k["state"]["points"]
    u, v = mo.centres(k["center"][0], k["half_width"][0], k["npix"][0]), mo.centres(k["center"][1], k["half_width"][1], k["npix"][1])
    assert all(np.any(u == p[i, 1]) and np.any(v == p[i, 2]) for i in range(3))
    assert ref("long-list")["count"].max() == 3000 > 4 * 256
    neg = ref("negative-T")
    assert np.all(neg["gas_temperature"] >= 0) and np.any(neg["dust_temperature"] < 0)
    assert {k["state"]["points"].shape[0] for n, k in c.items() if n.startswith("subset-n")} == {1, 2, 257}
    assert {k["npix"] for n, k in c.items() if n.startswith("cube_gas")} == set(mc.NPIX)
    assert {k["axes"] for n, k in c.items() if n.startswith("axes-")} == set(mc.AXES)


def _cxx():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_tile_walk_on_the_host(tmp_path, sanitize):
    """tests/host/map_check.cpp: spans, tile lists and the batched walk replayed with sphx_map_pair.h give every pixel the
    bits of the plain sum over all particles; the staging array is never read beyond a batch."""
    cxx = _cxx()
    if cxx is None:
        pytest.skip("no host C++ compiler on this machine")
    exe = str(tmp_path / "map_check")
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"]
    if sanitize:
        flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        ver = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
        if "clang" not in ver.lower():          # (GCC's runtimes, linked dynamically, insist on being loaded first)
            flags += ["-static-libasan", "-static-libubsan"]
    res = subprocess.run([cxx] + flags + ["-o", exe, os.path.join(ROOT, "tests", "host", "map_check.cpp")], capture_output=True, text=True)
    no_runtime = any(("cannot find" in ln or "no such file" in ln.lower()) and ("asan" in ln or "ubsan" in ln)
                     for ln in res.stderr.splitlines())
    if res.returncode != 0 and sanitize and no_runtime:
        pytest.skip("this compiler has no sanitizer runtimes: " + res.stderr.strip().splitlines()[-1])
    assert res.returncode == 0, res.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "sphx_map: 0 violations" in run.stdout
    broken = [ln for ln in run.stdout.splitlines() if ln.startswith("broken rule:")]
    assert broken and int(broken[0].split()[2]) > 0              # the check can fail
