"""GPU tests (-m gpu) of the sums the LDS passes do not finish because they are NaN already (sphx_settled.h, blob_pass):
pass 3 neither stages nor walks a blob whose rows' own m Pi is NaN, pass 2 goes on with the crossing-time term alone in a
wave whose rows' sums are all NaN.  The states are tests/settled_cases.py's (tests/test_settled_cases_cpu.py shows that
none is vacuous).  What is compared:
  - three fused steps in the four forms of test_step_loop_variants_are_bit_identical - LDS (default), LDS with the image
    squeezed to 100 slots (part of the references take the global-memory path), gathers in blob order (SPHX_LDS=0),
    gathers in storage order (SPHX_BLOB=0) - bit for bit, NaN for NaN, after the first and after the third step;
  - the counters visc_blobs_settled / pi_waves_settled (include/sphx.h), which prove a shortcut taken or not taken;
  - the array API's hydro_update (the gather kernels) against the oracle: identical NaN pattern, the finite rows within
    the per-row bound of tests/oracle_bounds.py.
The step does not hand out Pi or the viscous acceleration by themselves: they are compared through visc_heat, total_accel
and everything the update makes of them."""
import numpy as np
import pytest

import oracle_bounds as ob
import settled_cases as sc

pytestmark = pytest.mark.gpu

FORMS = (("lds", {}), ("lds_overflow", {"SPHX_BLOB_SLOTS": "100"}), ("blob_gather", {"SPHX_LDS": "0"}),
         ("storage_order", {"SPHX_BLOB": "0"}))
KEYS = ("points", "velocities", "total_accel", "E_internal", "T", "visc_heat", "sizes", "densities", "num_densities")
COUNTERS = ("visc_blobs_settled", "pi_waves_settled")


def _run_forms(state, K, monkeypatch, steps=(1, 2)):
    """-> {form: [(download, failures, counters) after each entry of `steps` more steps]}"""
    from sph_code_amd.sim import Simulation
    res = {}
    for name, env in FORMS:
        for k_, v in env.items():
            monkeypatch.setenv(k_, v)
        sim = Simulation(state, n_neigh=K)                 # a fresh context reads the switches
        seen = []
        for nst in steps:
            sim.step(nst, fixed_dt=sc.FIXED_DT)
            st = sim.stats()
            seen.append((sim.download(), sim.failures(), {c: int(st[c]) for c in COUNTERS}))
        res[name] = seen
        for k_ in env:
            monkeypatch.delenv(k_)
    return res


def _assert_forms_equal(res, label):
    ref = res["storage_order"]                             # the gather kernels in storage order
    for name in ("lds", "lds_overflow", "blob_gather"):
        for (d, f, _), (dr, fr, _) in zip(res[name], ref):
            for key in KEYS:
                assert np.array_equal(np.isnan(d[key]), np.isnan(dr[key])), (label, name, key, "NaN mask")
                assert np.array_equal(d[key], dr[key], equal_nan=True), (label, name, key)
            assert d["dt"] == dr["dt"], (label, name, d["dt"], dr["dt"])
            assert f == fr, (label, name, f, fr)


@pytest.mark.parametrize("K", sc.KS)
@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_settled_sums_equal_the_gather_forms(variant, K, monkeypatch):
    st, bad = sc.make_case(variant, K)
    res = _run_forms(st, K, monkeypatch)
    for name in res:
        print(variant, K, name, [(c, f["bad_accel"]) for _, f, c in res[name]])
    _assert_forms_equal(res, (variant, K))
    first = res["storage_order"][0][1]
    assert first["bad_accel"] >= sc.N_CLUMP                # the state does what it was built for: A's rows are NaN
    for name in ("lds", "lds_overflow"):
        c1, c3 = res[name][0][2], res[name][1][2]
        # clump A: 512 consecutive rows of the blob order hold three whole blobs - per launch of pass 3
        assert c1["visc_blobs_settled"] >= 3, (name, c1)
        assert c3["visc_blobs_settled"] >= 3 * 3, (name, c3)
        if K > 8:
            assert c1["pi_waves_settled"] > 0 and c3["pi_waves_settled"] > c1["pi_waves_settled"], (name, c1, c3)
        else:                                              # one batch of eight list positions: no batch left to shorten
            assert c3["pi_waves_settled"] == 0, (name, c3)
        # ... and not every blob: B's and C's are walked
        assert c1["visc_blobs_settled"] < 3 * sc.N_CLUMP // 128 - 4, (name, c1)
    for name in ("blob_gather", "storage_order"):          # the gather kernels have no such path
        assert all(v == 0 for _, _, c in res[name] for v in c.values()), (name, res[name][-1][2])


def test_healthy_clump_takes_no_shortcut(monkeypatch):
    st, _ = sc.make_case("centre", 40, clumps="B")
    res = _run_forms(st, 40, monkeypatch)
    _assert_forms_equal(res, "B alone")
    for name in res:
        for d, f, c in res[name]:
            assert c == {"visc_blobs_settled": 0, "pi_waves_settled": 0}, (name, c)
            assert f["bad_accel"] == 0 and np.isfinite(d["total_accel"]).all() and np.isfinite(d["visc_heat"]).all()


@pytest.fixture(scope="module")
def nsc():
    import sph_code_amd.compat as nsc_mod
    nsc_mod.context()            # raises if libsphx.so / the GPU is missing: no fallback
    return nsc_mod


@pytest.mark.parametrize("K", sc.KS)
@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_hydro_update_against_the_oracle(nsc, variant, K):
    """One call of the array API's hydro_update (the gather kernels: the unshortened sums) on the same states: the NaN
    pattern of visc_accel and visc_heat is the oracle's, the finite rows hold the per-row bound."""
    st, bad = sc.make_case(variant, K)
    idx, _, _, _, h = nsc.neighbors(st["points"], np.inf, K)
    args = sc.hydro_args_of(st, idx, h)
    out = nsc.hydro_update(*args)
    ref, scales = ob.hydro_reference(args)
    seen = ob.compare_hydro(out, ref, scales, "%s K=%d" % (variant, K), which=(1, 2), visc_nonfinite_ok=True)
    nan_row = np.isnan(out[1]).any(axis=1)
    assert nan_row[sc.A].all() and not nan_row[sc.B].any() and nan_row[sc.C].any() and not nan_row[sc.C].all()
    assert seen["visc_heat"] == int((~nan_row).sum()) > sc.N_CLUMP
