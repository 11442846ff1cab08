"""GPU tests (-m gpu) of pass 2 handing its rows on to pass 3 (sphx_blob.hip: PiPass::finish, blob_visc_kernel): in the
fused single-GPU step with the LDS passes, pass 2 writes pass 3's NaNs for the rows that are settled (sphx_settled.h)
and marks every blob that holds another row; pass 3 walks the marked blobs alone, and a launch that finds none returns at
once (sphx_stats.visc_launches_skipped; the blobs not walked count in visc_blobs_settled).  The states are
tests/settled_cases.py's.
What is compared:
  - the LDS forms against the gather kernels in storage order (SPHX_BLOB=0), bit for bit, NaN for NaN, dt and failure
    counters included, after one and after three steps - on states where every launch is skipped (clump A alone, whole
    and cut to 500 particles so that the last blob has pad rows), where none is (A + B, A + B + C, B alone), and on a
    polytrope of 20 000 at the reference's own dt;
  - the counters, which say whether a launch was skipped;
  - a context that goes from a healthy state to a NaN one and back: the marks of the last step do not leak;
  - the paths that do not hand on: the array API's hydro_update leaves the counter alone.
The step does not hand out the viscous acceleration by itself: "NaN in every row" is asserted on visc_heat and through
bad_accel (the update counts a row whose viscous acceleration is not finite), the rest through the bit equality."""
import numpy as np
import pytest

import settled_cases as sc

pytestmark = pytest.mark.gpu

FORMS = (("lds", {}), ("lds_overflow", {"SPHX_BLOB_SLOTS": "100"}), ("blob_gather", {"SPHX_LDS": "0"}),
         ("storage_order", {"SPHX_BLOB": "0"}))
LDS_FORMS = ("lds", "lds_overflow")
KEYS = ("points", "velocities", "total_accel", "E_internal", "T", "visc_heat", "sizes", "densities", "num_densities")
COUNTERS = ("visc_launches_skipped", "visc_blobs_settled", "pi_waves_settled")
STEPS = (1, 2)


def _seen(sim):
    st = sim.stats()
    return sim.download(), sim.failures(), {c: int(st[c]) for c in COUNTERS}


def _run(state, K, steps=STEPS, fixed_dt=sc.FIXED_DT, ctx=None):
    """-> [(download, failures, counters) after each entry of `steps` more steps]"""
    from sph_code_amd.sim import Simulation
    sim = Simulation(state, n_neigh=K, ctx=ctx)
    out = []
    for nst in steps:
        sim.step(nst, fixed_dt=fixed_dt)
        out.append(_seen(sim))
    return out


def _run_forms(state, K, monkeypatch, forms=FORMS, **kw):
    res = {}
    for name, env in forms:
        for k_, v in env.items():
            monkeypatch.setenv(k_, v)
        res[name] = _run(state, K, **kw)                   # a fresh context reads the switches
        for k_ in env:
            monkeypatch.delenv(k_)
    return res


def _assert_same(got, ref, label):
    assert len(got) == len(ref)
    for (d, f, _), (dr, fr, _) in zip(got, ref):
        for key in KEYS:
            assert np.array_equal(np.isnan(d[key]), np.isnan(dr[key])), (label, key, "NaN mask")
            assert np.array_equal(d[key], dr[key], equal_nan=True), (label, key)
        assert d["dt"] == dr["dt"], (label, d["dt"], dr["dt"])
        assert f == fr, (label, f, fr)


def _assert_forms_equal(res, label):
    for name in res:
        if name != "storage_order":
            _assert_same(res[name], res["storage_order"], (label, name))


def _head(state, n):
    """The first n particles of a state."""
    n0 = len(state["points"])
    return {k_: (v[:n].copy() if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == n0 else v)
            for k_, v in state.items()}


@pytest.mark.parametrize("K", (7, 40))
@pytest.mark.parametrize("n", (sc.N_CLUMP, 500))
def test_every_launch_is_skipped_where_every_row_is_nan(n, K, monkeypatch):
    """Clump A alone (every T < 0): 4 blobs per launch, with 500 particles the last one has 12 pad rows - which neither
    count as live nor get written."""
    st, _ = sc.make_case("centre", K, clumps="A")
    if n < sc.N_CLUMP:
        st = _head(st, n)
    res = _run_forms(st, K, monkeypatch)
    for name in res:
        print(n, K, name, [(c, f["bad_accel"]) for _, f, c in res[name]])
    _assert_forms_equal(res, ("A", n, K))
    done = 0
    for q, nst in enumerate(STEPS):
        done += nst
        for name in res:
            d, f, c = res[name][q]
            assert np.isnan(d["visc_heat"]).all(), (name, q)
            assert f["bad_accel"] == n * done and f["bad_energy"] == n * done, (name, q, f)
            if name in LDS_FORMS:
                assert c["visc_launches_skipped"] == done and c["visc_blobs_settled"] == 4 * done, (name, q, c)
            else:                                          # the gather kernels have no such path
                assert c["visc_launches_skipped"] == 0 and c["visc_blobs_settled"] == 0, (name, q, c)


@pytest.mark.parametrize("variant,clumps", [(v, "ABC") for v in sc.VARIANTS] + [("centre", "AB")])
def test_no_launch_is_skipped_while_a_row_is_live(variant, clumps, monkeypatch):
    K = 40
    st, _ = sc.make_case(variant, K, clumps=clumps)
    res = _run_forms(st, K, monkeypatch)
    for name in res:
        print(variant, clumps, name, [c for _, _, c in res[name]])
    _assert_forms_equal(res, (variant, clumps))
    for name in res:
        for _, _, c in res[name]:
            assert c["visc_launches_skipped"] == 0, (name, c)
    for name in LDS_FORMS:                                 # A's whole blobs are still not walked
        assert res[name][0][2]["visc_blobs_settled"] >= 3, (name, res[name][0][2])


def test_healthy_clump_skips_nothing(monkeypatch):
    st, _ = sc.make_case("centre", 40, clumps="B")
    res = _run_forms(st, 40, monkeypatch)
    _assert_forms_equal(res, "B alone")
    for name in res:
        for d, f, c in res[name]:
            assert all(v == 0 for v in c.values()), (name, c)
            assert f["bad_accel"] == 0 and np.isfinite(d["total_accel"]).all() and np.isfinite(d["visc_heat"]).all()


@pytest.mark.parametrize("order", ("BA", "AB"))
def test_the_marks_of_one_run_do_not_reach_the_next(order):
    """A healthy state (every row live) and a NaN one (none) one after the other on ONE context: the second run equals
    the same run on a context of its own, and each run skips what it skips alone - pass 2 writes every blob's mark anew
    in every step."""
    from sph_code_amd import _lib
    from sph_code_amd.sim import Simulation
    K = 40
    states = {q: sc.make_case("centre", K, clumps=q)[0] for q in "AB"}
    alone = {q: _run(states[q], K, steps=(2,)) for q in "AB"}
    for q in "AB":
        assert alone[q][0][2]["visc_launches_skipped"] == (2 if q == "A" else 0), (q, alone[q][0][2])
    ctx = _lib.Context()
    for q in order:
        sim = Simulation(states[q], n_neigh=K, ctx=ctx)
        before = int(ctx.stats()["visc_launches_skipped"])     # (whatever an upload makes of the counters)
        sim.step(2, fixed_dt=sc.FIXED_DT)
        got = [_seen(sim)]
        print(order, q, "before", before, got[0][2])
        _assert_same(got, alone[q], (order, q))
        assert got[0][2]["visc_launches_skipped"] - before == (2 if q == "A" else 0), (order, q, got[0][2])


MI355X_GRID = 512          # workgroups of the LDS passes' persistent grid: two per CU


@pytest.mark.parametrize("n", (200_000, 1_060_000))
def test_the_walk_of_the_marked_blobs_equals_the_gather_kernels(n, monkeypatch):
    """The mixed regime at sizes where a workgroup of pass 3 keeps several marked blobs: a polytrope with T < 0 on the
    side x < 0 - those rows and their neighbours are settled, the blobs of the other side are marked, more of them than
    the grid has workgroups.  1 060 000 particles are 8282 blobs: the count and the numbering of the marks take a second
    round of 8192.  Two steps of the tests' short dt, bit for bit against the gather kernels in storage order: a marked
    blob that nobody walked would keep the viscous sums of the step before (or what the buffer held), a blob walked
    twice costs nothing but is excluded by the numbering being a bijection (every marked blob is somebody's)."""
    import sph_code_amd.ics as ics
    st = ics.WORKLOADS["polytrope"](n, light=True)
    neg = st["points"][:, 0] < 0.0
    st["T"] = np.where(neg, -st["T"], st["T"])
    st["E_internal"] = np.where(neg, -st["E_internal"], st["E_internal"])
    forms = tuple(f for f in FORMS if f[0] in ("lds", "storage_order"))
    res = _run_forms(st, 40, monkeypatch, forms=forms, steps=(1, 1))
    _assert_forms_equal(res, ("half NaN", n))
    nblk = (((n + 63) // 64) * 64 + 127) // 128
    settled_before = 0
    for d, f, c in res["lds"]:
        settled = c["visc_blobs_settled"] - settled_before
        settled_before = c["visc_blobs_settled"]
        nan_rows = int(np.isnan(d["visc_heat"]).sum())
        print(n, "blobs", nblk, "not walked", settled, "walked", nblk - settled, "NaN rows", nan_rows, c)
        assert 0 < settled < nblk, (n, settled, nblk)
        assert nblk - settled > MI355X_GRID, (n, nblk - settled)      # some workgroup walks two marked blobs and more
        assert c["visc_launches_skipped"] == 0, c
        assert neg.sum() <= nan_rows < n, (n, nan_rows)
    if n > 1_000_000:
        assert nblk > 16 * 512                                        # the marks' second round (VISC_ROUND)


def test_a_real_flow_equals_the_gather_kernels(monkeypatch):
    """Polytrope of 20 000, the reference's own dt, four steps: whether the later steps skip at this size is not known
    in advance - the counter is printed, and bounded by "the first step has nothing settled"."""
    import sph_code_amd.ics as ics
    st = ics.WORKLOADS["polytrope"](20000)
    forms = tuple(f for f in FORMS if f[0] in ("lds", "storage_order"))
    res = _run_forms(st, 40, monkeypatch, forms=forms, steps=(4,), fixed_dt=0.0)
    _assert_forms_equal(res, "polytrope 20000")
    c = res["lds"][0][2]
    print("polytrope 20000, 4 steps:", c, res["lds"][0][1])
    assert 0 <= c["visc_launches_skipped"] <= 4 - 1, c
    assert res["storage_order"][0][2]["visc_launches_skipped"] == 0


def test_hydro_update_does_not_hand_on():
    """The array API's passes run on their own: the counter stays, the NaN pattern is the clumps'."""
    import sph_code_amd.compat as nsc
    ctx = nsc.context()
    K = 40
    st, _ = sc.make_case("centre", K)
    idx, _, _, _, h = nsc.neighbors(st["points"], np.inf, K)
    before = int(ctx.stats()["visc_launches_skipped"])
    out = nsc.hydro_update(*sc.hydro_args_of(st, idx, h))
    assert int(ctx.stats()["visc_launches_skipped"]) == before
    nan_row = np.isnan(out[1]).any(axis=1)
    assert nan_row[sc.A].all() and not nan_row[sc.B].any() and nan_row[sc.C].any() and not nan_row[sc.C].all()
    assert np.array_equal(np.isnan(out[2]), nan_row)
    # ... and on clump A alone, where the step skips every launch
    sa, _ = sc.make_case("centre", K, clumps="A")
    idx, _, _, _, h = nsc.neighbors(sa["points"], np.inf, K)
    out = nsc.hydro_update(*sc.hydro_args_of(sa, idx, h))
    assert int(ctx.stats()["visc_launches_skipped"]) == before
    assert np.isnan(out[1]).all() and np.isnan(out[2]).all()
