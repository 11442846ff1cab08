"""GPU checks of supernova_destruction (nsc:1211-1263; include/sphx.h sphx_supernova_destruction) against the NumPy
restatement tests/dust_oracle.py, to the bounds that module derives (1e-12 sum|term| per sum, 16 ulp per coefficient, the
cancellation of s^2 - r^2 near the edge of a grain's support, propagated to first order through the interpolation, the
cap and the final division).  No element is left out of any comparison, and the regime counts are compared for equality:
tests/test_dust_cpu.py shows that no decision of any input set used here lies within reach of the bound."""
import numpy as np
import pytest

import cool_fixture
import dust_fixture
import dust_oracle

pytestmark = pytest.mark.gpu

OUT = dust_oracle.OUTPUTS


def gpu(f, **over):
    import sph_code_amd.compat as nsc
    a, b, c = nsc.supernova_destruction(*dust_fixture.args(f), full=True, **dict(dust_fixture.opts(f), **over))
    return dict(frac_destruction=a, frac_reuptake=b, counts=c)


def check(f, o, what):
    got = gpu(f)
    for nm in OUT:
        print(what, nm, "worst |diff| / bound %.3g" % dust_oracle.worst_ratio(got[nm], o[nm], o[nm + "_bound"]))
    print(what, "counts", got["counts"], "restatement", o["counts"])
    for nm in OUT:
        dust_oracle.assert_within(nm, got[nm], o[nm], o[nm + "_bound"], what)
    assert got["counts"] == o["counts"], what
    return got


def check_set(f, what):
    o = dust_fixture.run_oracle(f)
    return check(f, o, what), o


@pytest.mark.parametrize("which", ["count", "fraction"])
def test_fixture(which):
    """The committed fixture under the reference's guard, and its high-density set under the fraction guard."""
    f = dust_fixture.load() if which == "count" else dust_fixture.fraction_set()
    o = dust_fixture.oracle(which)
    got = check(f, o, "fixture " + which)
    c = got["counts"]
    assert c["accepted"] > 0 and c["rejected_by_accumulation"] > 0 and (c["capped"] > 0) == (which == "fraction")
    if which == "count":
        # the reference's own capture: frac_reuptake's rows were added pairwise there, in list order here
        dust_oracle.assert_within("frac_destruction", got["frac_destruction"], f["ref_frac_destruction"], o["frac_destruction_bound"])
        dust_oracle.assert_within("frac_reuptake", got["frac_reuptake"], f["ref_frac_reuptake"], o["frac_reuptake_bound"])


def test_same_bits_on_every_call_and_inputs_untouched():
    import sph_code_amd.compat as nsc
    f = dust_fixture.fraction_set()
    a_ = [np.array(a, copy=True) for a in dust_fixture.args(f)]
    keep = [np.array(a, copy=True) for a in a_]
    kw = dust_fixture.opts(f)
    a = nsc.supernova_destruction(*a_, full=True, **kw)
    b = nsc.supernova_destruction(*a_, full=True, **kw)
    short = nsc.supernova_destruction(*a_, **kw)
    assert len(a) == 3 and len(short) == 2 and a[2] == b[2]
    for x, y in zip(a[:2], b[:2]):
        assert np.array_equal(x, y)
    for x, y in zip(a[:2], short):
        assert np.array_equal(x, y)
    for x, y in zip(a_, keep):
        assert np.array_equal(x, y)
    ms = nsc.dust_last_timing()
    assert set(ms) == {"upload", "reverse", "dust", "rows"} and all(v >= 0.0 for v in ms.values()) and ms["dust"] > 0.0


@pytest.mark.parametrize("K", dust_fixture.CLOUD_K)
def test_small_shapes(K):
    """N = K + 1, around the workgroup size and over several workgroups; S = 8, 15, 32 and both guards in turn."""
    lost = 0
    for name, f in dust_fixture.shape_clouds(K):
        got, _ = check_set(f, name)
        lost += got["counts"]["lost"]
    assert (lost > 0) == (K > 1)


def test_no_dust_at_all():
    """M = 0: nothing to sort, zeros out."""
    got, _ = check_set(dust_fixture.input_sets()["no dust"](), "no dust")
    assert np.all(got["frac_destruction"] == 0.0) and np.all(got["frac_reuptake"] == 0.0)
    assert not any(got["counts"].values())


def test_all_dust():
    f = dust_fixture.cloud(300, 7, 15, 9)
    f["particle_type"] = np.full(300, 2.0)
    got, _ = check_set(f, "all dust")
    assert np.all(got["frac_destruction"] == 0.0) and np.all(got["frac_reuptake"] == 0.0)
    assert not any(got["counts"].values())


@pytest.mark.parametrize("n,K", dust_fixture.SHORT)
def test_fewer_particles_than_columns(n, K):
    """Entries equal to N contribute nothing."""
    f = dust_fixture.short_cloud(n, K)
    assert n > K - 1 or np.any(f["neighbor"] == n)
    got, _ = check_set(f, "n=%d K=%d" % (n, K))
    if n < K:
        again = gpu(dict(f, neighbor=np.ascontiguousarray(f["neighbor"][:, :n])))
        for nm in OUT:
            assert np.array_equal(got[nm], again[nm]), nm
        assert got["counts"] == again["counts"]


@pytest.mark.parametrize("guard", ["count", "fraction"])
def test_hub_grain_in_more_rows_than_a_workgroup(guard):
    """One grain's slice of 600 pairs; the guard flips inside it."""
    f = dust_fixture.hub(guard)
    got, o = check_set(f, "hub " + guard)
    c = got["counts"]
    assert o["pairs"] == 600 and c["accepted"] > 120 and c["rejected_by_accumulation"] > 120
    assert np.all(got["frac_destruction"][1:] == 0.0) and np.all(got["frac_destruction"][0, 7:13] > 0.0)
    if guard == "fraction":
        assert np.all(got["frac_destruction"] < 1.0) and got["frac_destruction"][0].max() > 0.9


def test_selector_of_nothing_gives_zeros_and_a_given_one_is_used():
    f = dust_fixture.cloud(257, 7, 15, 5)
    got = gpu(f, species_curve=np.zeros(15, np.int32))
    assert np.all(got["frac_destruction"] == 0.0) and np.all(got["frac_reuptake"] == 0.0) and not any(got["counts"].values())
    got, _ = check_set(dust_fixture.extra("own selector"), "own selector")
    sc = np.array(dust_fixture.OWN_SELECTOR)
    assert np.all(got["frac_destruction"][:, sc == 0] == 0.0) and np.any(got["frac_destruction"][:, 14] > 0.0)


def test_crit_mass_and_critical_density_are_arguments():
    check_set(dust_fixture.extra("every grain above crit_mass"), "every grain above crit_mass")
    got, _ = check_set(dust_fixture.extra("no grain above crit_mass"), "no grain above crit_mass")
    assert np.all(got["frac_destruction"] == 0.0)
    check_set(dust_fixture.extra("another critical density"), "another critical density")


def test_status_codes_of_the_c_abi():
    import sph_code_amd.compat as nsc
    from sph_code_amd._lib import c_int32_p, dp, ip
    f = dust_fixture.cloud(64, 7, 15, 14)
    ctx = nsc.context()
    n, K, S = 64, 7, 15
    a = {k: np.ascontiguousarray(v) for k, v in f.items() if isinstance(v, np.ndarray)}
    sc = nsc.dust_species_curve(S)
    kv, kc, ks = (np.array(v, dtype=np.float64) for v in (nsc.DUST_KNOTS_V, nsc.DUST_KNOTS_C, nsc.DUST_KNOTS_SI))
    fd, fr = np.full((n, S), -7.0), np.full((n, S), -7.0)

    def call(n_=n, k_=K, s_=S, cm=f["crit_mass"], cd=f["critical_density"], guard=0, counts=None, **over):
        p = dict(pos=dp(a["points"]), vel=dp(a["velocities"]), nb=ip(a["neighbor"]), m=dp(a["mass"]), f=dp(a["f_un"]),
                 mu=dp(a["mu_array"]), sz=dp(a["sizes"]), dens=dp(a["densities"]), pt=dp(a["particle_type"]),
                 sc=sc.ctypes.data_as(c_int32_p), kv=dp(kv), kc=dp(kc), ks=dp(ks), fd=dp(fd), fr=dp(fr))
        p.update(over)
        return ctx.lib.sphx_supernova_destruction(ctx.h, n_, k_, s_, p["pos"], p["vel"], p["nb"], p["m"], p["f"], p["mu"], p["sz"],
                                                  p["dens"], p["pt"], cm, cd, p["sc"], p["kv"], p["kc"], p["ks"], guard, p["fd"],
                                                  p["fr"], counts)

    bad = [call(n_=0), call(n_=-1), call(k_=0), call(k_=65), call(s_=0), call(s_=33), call(cm=np.inf), call(cm=np.nan),
           call(cd=np.nan), call(cd=-np.inf), call(guard=2), call(guard=-1)]
    bad += [call(**{nm: None}) for nm in ("pos", "vel", "nb", "m", "f", "mu", "sz", "dens", "pt", "sc", "kv", "kc", "ks", "fd", "fr")]
    for code in (3, -1):
        sc_bad = sc.copy(); sc_bad[4] = code
        bad.append(call(sc=sc_bad.ctypes.data_as(c_int32_p)))
    kv_bad = kv.copy(); kv_bad[3] = np.nan
    kc_bad = kc.copy(); kc_bad[7] = np.inf
    kv_flat = kv.copy(); kv_flat[5] = kv_flat[4]
    bad += [call(kv=dp(kv_bad)), call(kc=dp(kc_bad)), call(kv=dp(kv_flat))]
    for rc in bad:
        assert rc == -1, rc                                                              # SPHX_E_ARG
    assert np.all(fd == -7.0) and np.all(fr == -7.0)                                      # nothing written
    assert ctx.lib.sphx_supernova_destruction(None, n, K, S, *([None] * 9), 1.0, 1.0, *([None] * 4), 0, None, None, None) == -1
    assert call() == 0 and np.all(fd >= 0.0) and np.all(fr >= 0.0)                        # counts NULL
    counts = np.full(5, -7, dtype=np.int64)
    assert call(counts=ip(counts)) == 0 and np.all(counts >= 0) and counts[0] == counts[1] + counts[2]
    ms = np.zeros(4)
    assert ctx.lib.sphx_dust_last_timing(ctx.h, dp(ms)) == 0 and np.all(ms >= 0.0) and ms[2] > 0.0
    assert ctx.lib.sphx_dust_last_timing(ctx.h, None) == -1


def test_a_call_between_two_rad_cooling_calls_leaves_their_bits():
    import sph_code_amd.compat as nsc
    c = cool_fixture.cloud(257, 7, 31)
    ca = cool_fixture.cloud_compat_args(c)
    f = dust_fixture.input_sets()["side call"]()
    first = nsc.rad_cooling(*ca, d=c["d"], full=True)
    mine = gpu(f)
    second = nsc.rad_cooling(*ca, d=c["d"], full=True)
    for x, y in zip(first, second):
        assert np.array_equal(x, y)
    again = gpu(f)
    for nm in OUT:
        assert np.array_equal(mine[nm], again[nm]), nm
    assert mine["counts"] == again["counts"] and mine["counts"]["lost"] > 0
