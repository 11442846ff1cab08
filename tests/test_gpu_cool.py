"""GPU checks of rad_cooling (nsc:1019-1176; include/sphx.h sphx_rad_cooling) against the reference's own captured
results (tests/golden/cool_*.npz) and the NumPy restatement tests/cool_oracle.py, to the bounds that module derives
(1e-12 sum|term| per re-ordered sum, 16 ulp per temperature coefficient, the cancellation of Weigh2 near the edge of the
support, all propagated to first order).  No element is left out of any comparison.

NOT YET RUN on an MI355X where this line stands; see DESIGN 5.10 for the state of the measurements."""
import os
import re

import numpy as np
import pytest

import cool_fixture
import cool_oracle
from conftest import ROOT

pytestmark = pytest.mark.gpu

OUT = cool_oracle.OUTPUTS


def wg():
    """Lanes of a workgroup of the kernels, as include/sphx.h documents it."""
    src = open(os.path.join(ROOT, "include", "sphx.h")).read()
    return int(re.search(r"#define\s+SPHX_COOL_WG\s+(\d+)", src).group(1))


def gpu(args, d):
    import sph_code_amd.compat as nsc
    return dict(zip(OUT, nsc.rad_cooling(*args, d=d, full=True)))


def check(got, ref, bounds, what):
    for nm in OUT:
        print(what, nm, "worst |diff| / bound %.3g" % cool_oracle.worst_ratio(got[nm], ref[nm], bounds[nm + "_bound"]))
    for nm in OUT:
        cool_oracle.assert_within(nm, got[nm], ref[nm], bounds[nm + "_bound"], what)


def check_cloud(c, what):
    o = cool_fixture.cloud_oracle(c)
    got = gpu(cool_fixture.cloud_compat_args(c), c["d"])
    check(got, o, o, what)
    return got, o


@pytest.mark.parametrize("case", cool_fixture.CASES)
def test_fixture(case):
    """Against the reference's captured values, the row table included; the bounds are the restatement's."""
    f = cool_fixture.load(case)
    o = cool_fixture.oracle(case)
    got = gpu(cool_fixture.compat_args(f), f["d"])
    check(got, {nm: f["ref_" + nm] for nm in OUT}, o, case)
    assert np.any(got["rec_array"][5] > 0.99) and np.all(got["energy"][f["particle_type"] == 0] != 0.0)


def cloud_sizes():
    w = wg()
    return sorted({255, 256, 257, 2049, w - 1, w, w + 1})


@pytest.mark.parametrize("K", [1, 2, 7, 40, 64])
def test_seeded_clouds(K):
    """N around the workgroup size, more than one workgroup, and K + 1."""
    for n in sorted(set(cloud_sizes() + [K + 1])):
        c = cool_fixture.cloud(n, K, 100 + K)
        got, o = check_cloud(c, "n=%d K=%d" % (n, K))
        if K > 1 and n > 8:
            assert np.any(got["energy"] != 0.0) and np.any(o["row_num_e"] > 0.0)


@pytest.mark.parametrize("n,K", [(1, 1), (3, 7), (7, 7), (40, 64)])
def test_fewer_particles_than_columns(n, K):
    """Entries equal to N contribute nothing."""
    c = cool_fixture.cloud(n, K, 7, dust=0.0, stars=0.0)
    assert n > K - 1 or np.any(c["neighbor"] == n)
    got, _ = check_cloud(c, "n=%d K=%d" % (n, K))
    if n < K:
        short = dict(c, neighbor=np.ascontiguousarray(c["neighbor"][:, :n]))
        again = gpu(cool_fixture.cloud_compat_args(short), c["d"])
        for nm in OUT:
            assert np.array_equal(got[nm], again[nm]), nm


def test_hub_particle_in_every_row_and_one_in_none():
    """A reverse slice far longer than a workgroup: particle 0 sits in every one of 2049 rows, the last particle in none."""
    n = 2049
    c = cool_fixture.cloud(n, 3, 21, dust=0.0, stars=0.0)
    j = np.arange(n)
    c["neighbor"] = np.stack([np.zeros(n, np.int64), 1 + j % (n - 3), 1 + (j + 1) % (n - 3)], axis=1)
    assert not np.any(c["neighbor"] == n - 1) and np.all(c["neighbor"][:, 0] == 0)
    c["f_un"][0, 3:6] = [0.1, 0.02, 0.12]
    c["d"] = float(6e16 / np.min((c["masses"] / cool_oracle.M_0) ** (1.0 / 3.0)))      # every pair inside the support
    got, o = check_cloud(c, "hub")
    assert got["rec_array"][5, 0] > 0.0 and got["energy"][0] != 0.0
    assert np.all(got["rec_array"][:, n - 1] == 0.0) and got["energy"][n - 1] == 0.0
    ft = np.ascontiguousarray(c["f_un"].T)
    assert np.array_equal(got["final_comp"][n - 1], (ft / np.sum(ft, axis=0)).T[n - 1])


def test_all_dust_and_neutral_clouds():
    c = cool_fixture.cloud(300, 7, 3)
    c["particle_type"] = np.full(300, 2.0)
    got, _ = check_cloud(c, "all dust")
    ft = np.ascontiguousarray(c["f_un"].T)
    assert np.array_equal(got["final_comp"], (ft / np.sum(ft, axis=0)).T)
    assert np.all(got["energy"] == 0.0) and np.all(got["rec_array"] == 0.0) and np.all(got["row_table"] == 0.0)
    c = cool_fixture.cloud(300, 7, 4, neutral=True)
    got, _ = check_cloud(c, "neutral")
    assert np.all(got["energy"] == 0.0) and np.all(got["rec_array"][3:6] == 0.0) and np.any(got["rec_array"][2] > 0.0)
    assert np.all(np.isfinite(got["final_comp"]))


def test_row_whose_only_gas_member_is_itself():
    c = cool_fixture.cloud(257, 7, 9, dust=0.0, stars=0.0)
    j = 5
    c["particle_type"][c["neighbor"][j, 1:]] = 2.0
    c["f_un"][j, 3:6] = [0.1, 0.02, 0.12]
    assert c["particle_type"][j] == 0.0
    got, o = check_cloud(c, "lonely row")
    assert o["row_contributes"][j] and np.all(got["row_table"][j, [1, 3, 4]] > 0.0)


def test_same_bits_on_every_call_and_inputs_untouched():
    import sph_code_amd.compat as nsc
    f = cool_fixture.load("sphere_dust_n2048_k40")
    args = [np.array(a, copy=True) if isinstance(a, np.ndarray) else a for a in cool_fixture.compat_args(f)]
    keep = [np.array(a, copy=True) if isinstance(a, np.ndarray) else a for a in args]
    a = nsc.rad_cooling(*args, d=f["d"], full=True)
    b = nsc.rad_cooling(*args, d=f["d"], full=True)
    short = nsc.rad_cooling(*args, d=f["d"])
    assert len(a) == 4 and len(short) == 3
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    for x, y in zip(a, short):
        assert np.array_equal(x, y)
    for x, y in zip(args, keep):
        assert np.array_equal(x, y)
    ms = nsc.cool_last_timing()
    assert set(ms) == {"upload", "rows", "gather", "download"} and all(v >= 0.0 for v in ms.values()) and ms["rows"] > 0.0


def test_module_d_is_picked_up():
    import sph_code_amd.compat as nsc
    c = cool_fixture.cloud(257, 7, 12)
    args = cool_fixture.cloud_compat_args(c)
    old = nsc.d
    try:
        nsc.d = None
        with pytest.raises(NameError):
            nsc.rad_cooling(*args)
        nsc.d = c["d"]
        a = nsc.rad_cooling(*args)
    finally:
        nsc.d = old
    b = nsc.rad_cooling(*args, d=c["d"])
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    o = nsc.rad_cooling(*args, d=0.5 * c["d"])
    assert not np.array_equal(o[1], b[1])


def test_f_un_passes_through_nan_to_num():
    c = cool_fixture.cloud(64, 7, 13, dust=0.0, stars=0.0)
    c["f_un"][3, 9] = np.nan
    c["f_un"][4, 5] = np.nan
    check_cloud(c, "nan in f_un")


def test_status_codes_of_the_c_abi():
    import sph_code_amd.compat as nsc
    from sph_code_amd._lib import dp, ip
    c = cool_fixture.cloud(64, 7, 14)
    ctx = nsc.context()
    n, K, S = 64, 7, 15
    a = {k: np.ascontiguousarray(v) for k, v in c.items() if isinstance(v, np.ndarray)}
    fin, en, rec = np.full((n, S), -7.0), np.full(n, -7.0), np.full((S, n), -7.0)

    def call(n_=n, k_=K, s_=S, dt=c["dt"], d=c["d"], table=None, **null):
        p = dict(pos=dp(a["positions"]), pt=dp(a["particle_type"]), m=dp(a["masses"]), f=dp(a["f_un"]), nb=ip(a["neighbor"]),
                 mu=dp(a["mu_array"]), T=dp(a["T"]), fin=dp(fin), en=dp(en), rec=dp(rec))
        p.update(null)
        return ctx.lib.sphx_rad_cooling(ctx.h, n_, k_, s_, p["pos"], p["pt"], p["m"], p["f"], p["nb"], p["mu"], p["T"], dt, d,
                                        p["fin"], p["en"], p["rec"], table)

    bad = [call(n_=0), call(n_=-1), call(k_=0), call(s_=5), call(dt=np.inf), call(dt=np.nan), call(d=np.nan), call(d=-np.inf)]
    bad += [call(**{nm: None}) for nm in ("pos", "pt", "m", "f", "nb", "mu", "T", "fin", "en", "rec")]
    for rc in bad:
        assert rc == -1, rc                                                              # SPHX_E_ARG
    assert np.all(fin == -7.0) and np.all(en == -7.0) and np.all(rec == -7.0)             # nothing written
    assert ctx.lib.sphx_rad_cooling(None, n, K, S, *([None] * 7), 1.0, 1.0, None, None, None, None) == -1
    assert call() == 0 and np.all(en >= 0.0) and np.all(rec >= 0.0)                       # row_table NULL
    table = np.full((n, 6), -7.0)
    assert call(table=dp(table)) == 0 and np.all(table >= 0.0)
    ms = np.zeros(4)
    assert ctx.lib.sphx_cool_last_timing(ctx.h, dp(ms)) == 0 and np.all(ms >= 0.0) and ms[1] > 0.0
    assert ctx.lib.sphx_cool_last_timing(ctx.h, None) == -1
