"""GPU tests (-m gpu) of the leapfrog/energy update that splits its rows in two classes (sphx_update_rows.h;
sphx_api.hip: step_sums, one_step): where pass 2 hands its rows on to pass 3 and neither drag nor gravity is on, it
leaves one byte per row - pass 3's result is settled (NaN) or not - in place of a settled row's four NaNs, and the update
takes a settled row's viscous sums as that constant without loading them; the other rows read what pass 3 summed.
sphx_stats.update_split_steps counts the steps that took this path.  The states are tests/settled_cases.py's.
What is compared, as tests/test_gpu_visc_skip.py does: the downloads bit for bit and NaN for NaN, dt and the failure
counters, against the gather kernels in storage order (SPHX_BLOB=0), which do not hand on and run the one update launch
  - on states where every row is settled (clump A, whole and cut to 500 particles), none is (clump B), and where blobs
    hold rows of both classes (A + B + C in every variant) - K = 7 and K = 40;
  - several steps in one step() call against the same steps as single calls;
  - healthy -> NaN -> healthy on ONE context: the bytes of one run do not reach the next;
  - download() straight after such a step: visc_heat is NaN exactly where the reference's is, although neither pass
    stored it there;
  - the counter: the number of steps on the default path; 0 with SPHX_BLOB=0, SPHX_LDS=0, drag or gravity, whose
    results are the reference's bits as before;
  - a polytrope of 20 000 at the reference's own dt (worked out in the update from pass 2's vote), three steps."""
import numpy as np
import pytest

import settled_cases as sc

pytestmark = pytest.mark.gpu

KEYS = ("points", "velocities", "total_accel", "E_internal", "T", "visc_heat", "sizes", "densities", "num_densities")
STEPS = (1, 2)
REF_ENV = {"SPHX_BLOB": "0"}
KS = (7, 40)


def _seen(sim):
    return sim.download(), sim.failures(), int(sim.stats()["update_split_steps"])


def _run(state, K, steps=STEPS, fixed_dt=sc.FIXED_DT, ctx=None, **sim_kw):
    """-> [(download, failures, split steps) after each entry of `steps` more steps]"""
    from sph_code_amd.sim import Simulation
    sim = Simulation(state, n_neigh=K, ctx=ctx, **sim_kw)
    out = []
    for nst in steps:
        sim.step(nst, fixed_dt=fixed_dt)
        out.append(_seen(sim))
    return out


def _run_env(env, monkeypatch, *a, **kw):
    for k_, v in env.items():
        monkeypatch.setenv(k_, v)
    try:
        return _run(*a, **kw)                              # a fresh context reads the switches
    finally:
        for k_ in env:
            monkeypatch.delenv(k_)


_states, _refs = {}, {}


def _state(variant, K, clumps, n=None):
    key = (variant, K, clumps, n)
    if key not in _states:
        st, _ = sc.make_case(variant, K, clumps=clumps)
        if n is not None:
            n0 = len(st["points"])
            st = {k_: (v[:n].copy() if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == n0 else v)
                  for k_, v in st.items()}
        _states[key] = st
    return _states[key]


def _reference(key, state, K, monkeypatch, **kw):
    """The gather kernels in storage order: computed once per state, shared, left unchanged."""
    if key not in _refs:
        _refs[key] = _run_env(REF_ENV, monkeypatch, state, K, **kw)
        for _, _, split in _refs[key]:
            assert split == 0, (key, split)                # SPHX_BLOB=0 does not hand on: no bytes
    return _refs[key]


def _assert_same(got, ref, label):
    assert len(got) == len(ref)
    for (d, f, _), (dr, fr, _) in zip(got, ref):
        for key in KEYS:
            assert np.array_equal(np.isnan(d[key]), np.isnan(dr[key])), (label, key, "NaN mask")
            assert np.array_equal(d[key], dr[key], equal_nan=True), (label, key)
        assert d["dt"] == dr["dt"], (label, d["dt"], dr["dt"])
        assert f == fr, (label, f, fr)


def _assert_split(got, steps=STEPS):
    done = 0
    for (_, _, split), nst in zip(got, steps):
        done += nst
        assert split == done, (split, done)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n", (sc.N_CLUMP, 500))
def test_every_row_settled(n, K, monkeypatch):
    """Clump A alone (every T < 0): no row loads a viscous sum; with 500 particles the last blob has 12 pad rows, which
    have no byte and no update."""
    st = _state("centre", K, "A", n if n < sc.N_CLUMP else None)
    ref = _reference(("A", n, K), st, K, monkeypatch)
    got = _run(st, K)
    _assert_same(got, ref, ("A", n, K))
    _assert_split(got)
    done = 0
    for (d, f, _), nst in zip(got, STEPS):
        done += nst
        assert np.isnan(d["visc_heat"]).all()
        assert f["bad_accel"] == n * done and f["bad_energy"] == n * done, f


@pytest.mark.parametrize("K", KS)
def test_no_row_settled(K, monkeypatch):
    """Clump B alone: every byte is written, none is set."""
    st = _state("centre", K, "B")
    ref = _reference(("B", K), st, K, monkeypatch)
    got = _run(st, K)
    _assert_same(got, ref, ("B", K))
    _assert_split(got)
    if K == 40:       # (at K = 7 a few rows of the healthy clump are NaN by themselves, in the reference as well)
        for d, f, _ in got:
            assert f["bad_accel"] == 0 and np.isfinite(d["visc_heat"]).all() and np.isfinite(d["total_accel"]).all()


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("variant", sc.VARIANTS)
def test_blobs_with_rows_of_both_classes(variant, K, monkeypatch):
    """A + B + C: C's blobs hold settled and live rows side by side.  A live row taken as settled loses its viscous
    force, a settled row taken as live reads what nobody stored: either breaks the bit equality of the state."""
    st = _state(variant, K, "ABC")
    ref = _reference(("ABC", variant, K), st, K, monkeypatch)
    got = _run(st, K)
    _assert_same(got, ref, ("ABC", variant, K))
    _assert_split(got)
    nan = np.isnan(got[0][0]["visc_heat"])
    assert nan[sc.A].all() and nan[sc.C].any() and not nan[sc.C].all()
    if K == 40:       # (at K = 7 a few rows of the healthy clump are NaN by themselves, in the reference as well)
        assert not nan[sc.B].any()


@pytest.mark.parametrize("K", KS)
def test_steps_in_one_call_and_as_single_calls(K, monkeypatch):
    """Three steps in one step() call and the same as three calls: equal to each other and to the reference."""
    st = _state("centre", K, "ABC")
    ref = _reference(("ABC", "centre", K, "3"), st, K, monkeypatch, steps=(3,))
    one = _run(st, K, steps=(3,))
    single = _run(st, K, steps=(1, 1, 1))
    _assert_same(one, ref, "one call")
    _assert_same(single[-1:], ref, "single calls")
    _assert_same(single[-1:], one, "single calls against one call")
    assert one[0][2] == 3 and [s for _, _, s in single] == [1, 2, 3]


@pytest.mark.parametrize("K", KS)
def test_the_bytes_of_one_run_do_not_reach_the_next(K, monkeypatch):
    """Healthy (no byte set at K = 40, a few at K = 7), NaN (every byte set), healthy again on ONE context: each run
    equals the reference of its state - pass 2 writes every row's byte anew in every step."""
    from sph_code_amd import _lib
    states = {q: _state("centre", K, q) for q in "AB"}
    refs = {"A": _reference(("A", sc.N_CLUMP, K), states["A"], K, monkeypatch),
            "B": _reference(("B", K), states["B"], K, monkeypatch)}
    ctx = _lib.Context()
    for q in "BAB":
        before = int(ctx.stats()["update_split_steps"])
        got = _run(states[q], K, ctx=ctx)
        _assert_same(got, refs[q], ("BAB", q))
        assert got[-1][2] - before == sum(STEPS), (q, before, got[-1][2])


@pytest.mark.parametrize("K", KS)
def test_download_straight_after_a_step_by_bytes(K, monkeypatch):
    """Neither pass stores the settled rows' viscous heat in such a step: the download fills the NaNs in - once; a
    second download sees the same."""
    from sph_code_amd.sim import Simulation
    st = _state("dust", K, "ABC")
    ref = _reference(("ABC", "dust", K), st, K, monkeypatch)
    sim = Simulation(st, n_neigh=K)
    sim.step(1, fixed_dt=sc.FIXED_DT)
    assert int(sim.stats()["update_split_steps"]) == 1
    d1, d2 = sim.download(), sim.download()
    want = ref[0][0]["visc_heat"]
    for d in (d1, d2):
        assert np.array_equal(np.isnan(d["visc_heat"]), np.isnan(want))
        assert np.array_equal(d["visc_heat"], want, equal_nan=True)
    assert np.isnan(want).any() and not np.isnan(want).all()


@pytest.mark.parametrize("name,env,sim_kw", [("blob_gather", {"SPHX_LDS": "0"}, {}),
                                             ("drag", {}, {"with_drag": True}),
                                             ("gravity", {}, {"gravity": "direct"})])
@pytest.mark.parametrize("K", KS)
def test_the_other_paths_keep_the_update_as_it_was(name, env, sim_kw, K, monkeypatch):
    """Without the LDS passes nothing is handed on, and with drag or gravity pass 2 stores the NaNs as before: the
    counter stays 0, and the results are those of the gather kernels in storage order with the same options."""
    st = _state("centre", K, "ABC")
    ref = _reference(("ABC", "centre", K, name), st, K, monkeypatch, **sim_kw)
    got = _run_env(env, monkeypatch, st, K, **sim_kw)
    _assert_same(got, ref, name)
    for _, _, split in got:
        assert split == 0, (name, split)


def test_a_real_flow_at_the_reference_dt(monkeypatch):
    """Polytrope of 20 000, the reference's own dt, three steps: the update works dt out of pass 2's vote, and its
    thread 0 leaves it for the host whatever row 0's class is."""
    import sph_code_amd.ics as ics
    st = ics.WORKLOADS["polytrope"](20000)
    ref = _reference("polytrope 20000", st, 40, monkeypatch, steps=(3,), fixed_dt=0.0)
    got = _run(st, 40, steps=(3,), fixed_dt=0.0)
    _assert_same(got, ref, "polytrope 20000")
    print("polytrope 20000, 3 steps: dt", got[0][0]["dt"], got[0][1], "NaN rows", int(np.isnan(got[0][0]["visc_heat"]).sum()))
    assert got[0][2] == 3
    assert got[0][0]["dt"] > 0.0
