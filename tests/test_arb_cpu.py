"""CPU-side checks of the arbitrary-point samplers (nsc:1422-1527): the NumPy restatement tests/arb_oracle.py against
the reference's own outputs (tests/golden/arb_*.npz), the gate and mask quirks, and the public surface."""
import inspect

import numpy as np
import pytest

import arb_oracle
from conftest import load_golden

CASES = ["sphere_dust_n2048_k40", "cube_gas_n2048_k40", "condensed_n1024_k40"]


def load_case(case):
    g, a = load_golden(case), load_golden("arb_" + case)
    return g, a


def oracle_for(g, a, tag, **over):
    kw = dict(points=g["points"], mass=g["mass"], particle_type=g["particle_type"], sizes=g["nb_h"], T=g["T"],
              n_part=a["n_part"], value=a["photoionization"], d=float(g["loop_d"]), m_0=float(g["const_m_0"]),
              arb_points=a["arb_points"], row_start=a[tag + "_row_start"], members=a[tag + "_members"])
    kw.update(over)
    return arb_oracle.fields(**kw)


@pytest.mark.parametrize("tag", ["ref", "exact"])
@pytest.mark.parametrize("case", CASES)
def test_oracle_matches_reference_outputs(case, tag):
    g, a = load_case(case)
    o = oracle_for(g, a, tag)
    for name in arb_oracle.FIELDS:
        arb_oracle.assert_within(name, o[name], a[tag + "_" + name], o[name + "_bound"], what="%s %s" % (case, tag))
    # the fixture exercises what it is meant to: contributing points, gate zeros, NaNs from empty photoionization sums
    assert (a[tag + "_density"] > 0).sum() > 50
    assert (np.diff(a[tag + "_row_start"]) <= 1).sum() >= int(a["n_far"])


@pytest.mark.parametrize("case", CASES)
def test_fixture_points(case):
    g, a = load_case(case)
    n_r, n_on, n_far = int(a["n_random"]), int(a["n_on"]), int(a["n_far"])
    q = a["arb_points"]
    assert q.shape == (n_r + n_on + n_far, 3)
    on = q[n_r:n_r + n_on]
    assert all((g["points"] == p).all(axis=1).any() for p in on)
    lo, hi = g["points"].min(axis=0), g["points"].max(axis=0)
    far = q[n_r + n_on:]
    gap = np.maximum(np.maximum(lo - far, far - hi), 0.0)
    assert (np.sqrt((gap ** 2).sum(axis=1)) > float(a["radius"])).all()
    assert float(a["radius"]) == float(np.max(g["nb_h"]))
    assert np.isnan(a["photoionization"]).sum() > 0 and (a["n_part"] > 0).all()


@pytest.mark.parametrize("case", CASES)
def test_exact_list_is_the_brute_force_ball(case):
    g, a = load_case(case)
    rs, mem = arb_oracle.brute_ball(g["points"], a["arb_points"], float(a["radius"]))
    assert np.array_equal(rs, a["exact_row_start"].astype(np.int64))
    ers, emem = a["exact_row_start"], a["exact_members"]
    for j in range(len(rs) - 1):
        assert np.array_equal(mem[rs[j]:rs[j + 1]], np.sort(emem[ers[j]:ers[j + 1]])), j


def test_gate_rows_of_length_0_and_1_give_zero():
    g, a = load_case("cube_gas_n2048_k40")
    q = g["points"][:3].copy()                 # on particles: a one-member row would contribute if it were summed
    rows = [[], [1], [2, 5, 9]]
    rs, mem = arb_oracle.to_csr(rows)
    o = oracle_for(g, a, "ref", arb_points=q, row_start=rs, members=mem)
    for name in arb_oracle.FIELDS:
        assert o[name][0] == 0.0 and o[name][1] == 0.0, name
        assert o[name + "_bound"][0] == 0.0 and o[name + "_bound"][1] == 0.0
    assert o["density"][2] > 0.0
    assert list(o["count"]) == [0, 1, 3]


def test_temperature_mask_is_the_numerators_sign():
    """temperature_arb masks on a = Wg g T > 0 (nsc:1480): a particle with T = 0 leaves BOTH sums, although its weight
    is positive; density_arb still counts it."""
    g, a = load_case("cube_gas_n2048_k40")
    gas = np.nonzero(g["particle_type"] == 0)[0][:3]
    q = g["points"][gas[:1]].copy()
    T = g["T"].copy()
    T[gas[0]] = 0.0                             # the particle the point sits on: the largest weight of the row
    others = np.argsort(((g["points"] - q[0]) ** 2).sum(axis=1))[:12]
    rs, mem = arb_oracle.to_csr([others])
    o = oracle_for(g, a, "ref", arb_points=q, row_start=rs, members=mem, T=T)
    o_all = oracle_for(g, a, "ref", arb_points=q, row_start=rs, members=mem)
    assert o["density"][0] == o_all["density"][0] > 0.0
    rest = others[others != gas[0]]
    rs2, mem2 = arb_oracle.to_csr([rest])
    o_rest = oracle_for(g, a, "ref", arb_points=q, row_start=rs2, members=mem2, T=T)
    assert o["temperature"][0] == o_rest["temperature"][0]
    assert o["temperature"][0] != o_all["temperature"][0]


def test_library_and_compat_offer_the_arb_family():
    import sph_code_amd._lib as L
    import sph_code_amd.compat as nsc
    lib = L.load_library()
    for nm in ("sphx_arb_fields", "sphx_arb_fields_list", "sphx_state_sample"):
        assert hasattr(lib, nm), "libsphx.so does not export %s" % nm
        assert nm in L.SIGNATURES
    want = {
        "neighbors_arb": ["points", "arb_points", "sizes"],
        "density_arb": ["points", "arb_points", "mass", "particle_type", "narb"],
        "dust_density_arb": ["points", "arb_points", "mass", "particle_type", "sizes", "narb"],
        "temperature_arb": ["points", "arb_points", "mass", "particle_type", "T", "narb"],
        "dust_temperature_arb": ["points", "arb_points", "mass", "particle_type", "sizes", "T", "narb"],
        "photoionization_arb": ["points", "arb_points", "mass", "N_PART", "photoionization", "particle_type", "narb"],
    }
    for name, args in want.items():
        params = list(inspect.signature(getattr(nsc, name)).parameters.values())
        pos = [p.name for p in params if p.default is inspect.Parameter.empty]
        assert pos == args, (name, pos)
        if name != "neighbors_arb":
            assert params[-1].name == "d" and params[-1].default is None
    from sph_code_amd.sim import Simulation
    from sph_code_amd import ics
    assert callable(Simulation.sample) and callable(ics.slice_points)


def test_slice_points():
    from sph_code_amd import ics
    q = ics.slice_points(center=(1.0, 2.0, 3.0), normal_axis=2, extent=(4.0, 2.0), shape=(5, 3))
    assert q.shape == (5, 3, 3)
    assert (q[..., 2] == 3.0).all()
    assert q[0, 0, 0] == pytest.approx(1.0 - 2.0) and q[-1, 0, 0] == pytest.approx(1.0 + 2.0)
    assert q[0, 0, 1] == pytest.approx(2.0 - 1.0) and q[0, -1, 1] == pytest.approx(2.0 + 1.0)
    q1 = ics.slice_points((0.0, 0.0, 0.0), 0, 2.0, (4, 4))
    assert (q1[..., 0] == 0.0).all() and q1[..., 1].min() == -1.0 and q1[..., 2].max() == 1.0
