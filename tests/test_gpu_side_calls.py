"""GPU checks of what the three side families - the arb samplers, rad_transfer and rad_cooling - share on the host side of
one context: the scan and its scratch, the read-back slots at the head of the pinned block, the upload / download tables,
the stage timer, and the saved and restored host state of a grid build between two steps.  Nothing here measures a value
against a yardstick (test_gpu_arb.py, test_gpu_rad.py and test_gpu_cool.py do): every comparison is bit for bit between
two calls of the same code on the same inputs, with calls of the other families in between.

NOT YET RUN on an MI355X where this line stands (no GPU could be obtained); DESIGN 5.8 says what has run."""
import numpy as np
import pytest

import cool_fixture
import rad_fixture
from conftest import load_golden

pytestmark = pytest.mark.gpu

CASE = "condensed_n1024_k40"                 # N = 1024, K = 40
M_ARB = 65                                   # one more than a workgroup of the grid kernel
N_SRC, N_DST = 3, 5
TIMING_KEYS = {"arb": ("upload", "build", "kernels", "download"), "rad": ("upload", "columns", "deposit", "download"),
               "cool": ("upload", "rows", "gather", "download")}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def call_arb(nsc):
    """Grid form on a ball of its own (nothing held from an earlier call is reused) and list form -> list of arrays."""
    g, a = load_golden(CASE), load_golden("arb_" + CASE)
    q = np.ascontiguousarray(a["arb_points"][:M_ARB])
    kw = dict(sizes=g["nb_h"], T=g["T"], N_PART=a["n_part"], photoionization=a["photoionization"], d=float(g["loop_d"]),
              with_stats=True)
    rs, mem = a["ref_row_start"].astype(np.int64), a["ref_members"].astype(np.int64)
    rows = [mem[rs[j]:rs[j + 1]] for j in range(M_ARB)]
    out = []
    for narb in (nsc.neighbors_arb(g["points"], q, g["nb_h"]), rows):
        got = nsc.arb_fields(g["points"], q, g["mass"], g["particle_type"], narb, **kw)
        out += [got[f] for f in nsc.ARB_FIELDS] + [got["count"], np.array([got["candidates"]], np.int64)]
    assert np.count_nonzero(out[0]) > 0 and out[6][0] > 0
    return out


def call_rad(nsc):
    f = rad_fixture.load(CASE)
    return list(nsc.rad_transfer(f["positions"], f["ptypes"], f["masses"], f["sizes"], f["cross_array"], f["mu_array"],
                                 f["sources"][:N_SRC], f["luminosities"][:N_SRC], f["targets"][:N_DST], f["dt"], full=True))


def call_cool(nsc):
    f = cool_fixture.load(CASE)
    return list(nsc.rad_cooling(*cool_fixture.compat_args(f), d=f["d"], full=True))


CALLS = {"arb": call_arb, "rad": call_rad, "cool": call_cool}


def timings(nsc):
    return {"arb": nsc.arb_last_timing(), "rad": nsc.rad_last_timing(), "cool": nsc.cool_last_timing()}


def test_interleaved_families_on_one_context():
    import sph_code_amd.compat as nsc
    kept = {fam: CALLS[fam](nsc) for fam in ("arb", "rad", "cool")}
    for step, fam in enumerate(("cool", "arb", "rad", "arb", "cool", "rad")):
        got = CALLS[fam](nsc)
        assert len(got) == len(kept[fam])
        for i, (x, y) in enumerate(zip(got, kept[fam])):
            assert same_bits(x, y), "call %d (%s): output %d differs from the family's first call" % (step, fam, i)


def test_timers_are_per_family():
    import sph_code_amd.compat as nsc
    from sph_code_amd._lib import dp, ip
    for fam in ("arb", "rad", "cool"):
        CALLS[fam](nsc)
    for fam in ("rad", "arb", "cool"):
        before = timings(nsc)
        CALLS[fam](nsc)
        after = timings(nsc)
        assert tuple(after[fam]) == TIMING_KEYS[fam]
        assert all(np.isfinite(v) and v >= 0.0 for v in after[fam].values()), after[fam]
        for other in ("arb", "rad", "cool"):
            if other != fam:
                assert after[other] == before[other], (fam, other)
    # A call that fails its argument check returns before its family's timer starts: the previous timing is kept.
    c = nsc.context()
    before = timings(nsc)
    assert all(sum(t.values()) > 0.0 for t in before.values())          # (kept is not zeroed)
    f, r, g = cool_fixture.load(CASE), rad_fixture.load(CASE), load_golden(CASE)
    n, S = f["positions"].shape[0], f["f_un"].shape[1]
    fin, en, rec = np.zeros((n, S)), np.zeros(n), np.zeros((S, n))
    pos, pt, m, mu, T = (np.ascontiguousarray(f[k]) for k in ("positions", "particle_type", "masses", "mu_array", "T"))
    assert c.lib.sphx_rad_cooling(c.h, n, 0, S, dp(pos), dp(pt), dp(m), dp(np.ascontiguousarray(f["f_un"])), ip(f["neighbor"]),
                                  dp(mu), dp(T), f["dt"], f["d"], dp(fin), dp(en), dp(rec), None) == -1          # K = 0
    src, dst, lum = (np.ascontiguousarray(r[k]) for k in ("sources", "targets", "luminosities"))
    assert c.lib.sphx_rad_transfer(c.h, n, dp(pos), dp(r["ptypes"]), dp(r["masses"]), dp(r["sizes"]), dp(r["cross_array"]),
                                   dp(r["mu_array"]), N_SRC, dp(src), dp(lum), N_DST, dp(dst), 1.0, 5, dp(en), None, None, None,
                                   None, None) == -1                                                          # unknown mode
    assert c.lib.sphx_arb_fields(c.h, 0, dp(g["points"]), dp(g["mass"]), dp(g["particle_type"]), None, None, None, None, 1.0,
                                 N_DST, dp(dst), 1.0, dp(en), None, None, None, None, None, None, 0) == -1    # n = 0
    assert timings(nsc) == before
    # A call that fails behind its argument check - here: no gas particle, found on the device - leaves its own family's
    # timing zeroed and the others' alone.
    with pytest.raises(ValueError, match="ptypes == 0"):
        nsc.rad_transfer(r["positions"], np.full(n, 2.0), r["masses"], r["sizes"], r["cross_array"], r["mu_array"], src[:N_SRC],
                         lum[:N_SRC], dst, r["dt"])
    after = timings(nsc)
    assert all(v == 0.0 for v in after["rad"].values())
    assert after["arb"] == before["arb"] and after["cool"] == before["cool"]


def test_all_three_between_steps_leave_the_loop_alone(monkeypatch):
    """step, step, then a sample, a rad_transfer on the resident state and compat.rad_cooling on the downloaded arrays - all
    three on the Simulation's own context - and a third step: the bits of a twin that took three steps and nothing else."""
    import sph_code_amd.compat as nsc
    from sph_code_amd import _lib
    from sph_code_amd.sim import Simulation
    g = load_golden("cube_gas_n2048_k40")
    K, d = 40, float(g["loop_d"])
    n = g["points"].shape[0]
    rs = np.random.RandomState(29)
    cross = 10.0 ** rs.uniform(-25.0, -21.0, n)
    lum = 10.0 ** rs.uniform(0.0, 4.0, N_SRC)
    ctxs = [_lib.Context(), _lib.Context()]
    try:
        for ctx in ctxs:
            ctx.set_constants(k_B=nsc.k, amu=nsc.amu, m_h=nsc.m_h, m_0=nsc.m_0, dt_0=nsc.dt_0,
                              solar_luminosity=nsc.solar_luminosity, c=nsc.c)
        sim, twin = (Simulation(g, n_neigh=K, ctx=ctx) for ctx in ctxs)
        for s in (sim, twin):
            s.step(1)
            s.step(1)
        st = sim.download()
        lo, hi = st["points"].min(axis=0), st["points"].max(axis=0)
        q = np.ascontiguousarray(lo + rs.rand(M_ARB, 3) * (hi - lo))
        sampled = sim.sample(q, d, fields=("density", "temperature"), with_stats=True)
        assert np.count_nonzero(sampled["density"]) > 0
        src, dst = st["points"][:N_SRC].copy(), st["points"][100:100 + N_DST].copy()
        lf2 = sim.rad_transfer(src, lum, dst, cross, st["dt"])[0]
        assert lf2.shape == (n,) and np.count_nonzero(lf2) > 0
        monkeypatch.setattr(nsc, "_ctx", ctxs[0])            # compat's calls now run on the Simulation's context
        final = nsc.rad_cooling(st["points"], g["particle_type"], g["mass"], st["sizes"], cross, g["f_un"],
                                g["nb_idx"].astype(np.int64), g["mu_array"], np.abs(st["T"]), st["dt"], d=d)[0]
        assert final.shape == g["f_un"].shape
        monkeypatch.undo()
        sim.step(1)
        twin.step(1)
        a, b = sim.download(), twin.download()
        for key in ("points", "velocities", "total_accel", "E_internal", "T", "sizes", "densities", "num_densities",
                    "visc_heat", "pressure"):
            assert same_bits(a[key], b[key]), key
        assert a["dt"] == b["dt"]
    finally:
        for ctx in ctxs:
            ctx.close()
