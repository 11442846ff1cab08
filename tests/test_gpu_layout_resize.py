"""GPU check that the side families carve their grow-only buffers by the call's n, not by the buffers' capacity
(sph-code_amd/csrc/sphx_carve.h): on one context a family is called at n = 257, at n = 6 inside the buffers the first call
left (n mod 4 = 2, K = 7 > n: the fixtures' short-cloud form), and at n = 257 again.  The third result has the bits of the
first, and the n = 6 result has the bits of the same call on a context that has allocated nothing yet.  What the carver itself
guarantees: tests/test_carve_cpu.py; the families against their oracles: their own suites."""
import numpy as np
import pytest

import chem_fixture
import cool_fixture
import dust_fixture

pytestmark = pytest.mark.gpu

BIG, SMALL, K = 257, 6, 7


def same_bits(a, b):
    """Equal bit for bit, a NaN equal to a NaN; tuples, lists and dicts member by member."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same_bits(a[k_], b[k_]) for k_ in a)
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def cool_call(n):
    import sph_code_amd.compat as nsc
    c = cool_fixture.cloud(n, K, 700 + n)
    return nsc.rad_cooling(*cool_fixture.cloud_compat_args(c), d=c["d"], full=True)


def dust_call(n):
    import sph_code_amd.compat as nsc
    f = dust_fixture.short_cloud(n, K) if n <= K else dust_fixture.cloud(n, K, 15, 309)
    return nsc.supernova_destruction(*dust_fixture.args(f), full=True, **dust_fixture.opts(f))


def chem_call(n):
    import sph_code_amd.compat as nsc
    f = chem_fixture.short_cloud(n, K) if n <= K else chem_fixture.cloud(n, K, 15, chem_fixture.SEEDS["n=257 K=7 S=15"])
    tables = {nm: f[nm] for nm in chem_fixture.TABLES}
    return nsc.chemisputtering_2(*chem_fixture.args(f), full=True, d=f["d"], dt=f["dt"], **tables)


def seeded(n):
    """Plain seeded arrays: masses about a solar mass, the three types, T, ages, 15 species, velocities, a list with entries
    n (missing) where n <= K, densities and sizes."""
    import sph_code_amd.compat as nsc
    rs = np.random.RandomState(4100 + n)
    pt = rs.choice([0.0, 1.0, 2.0], n, p=[0.6, 0.2, 0.2])
    pt[:3] = (0.0, 1.0, 2.0)
    nb = np.full((n, K), n, dtype=np.int64)
    kk = min(K, n)
    nb[:, :kk] = np.argsort(rs.rand(n, n), axis=1)[:, :kk]
    return dict(mass=nsc.solar_mass * 10.0 ** rs.uniform(-1.0, 1.0, n), particle_type=pt, T=10.0 ** rs.uniform(1.0, 4.0, n),
                star_ages=rs.uniform(0.0, 1e15, n), f_un=rs.rand(n, 15), velocities=rs.normal(0.0, 1e3, (n, 3)),
                total_accel=rs.normal(0.0, 1e-9, (n, 3)), E_internal=10.0 ** rs.uniform(30.0, 33.0, n), neighbor=nb,
                densities=10.0 ** rs.uniform(-20.0, -18.0, n), densities_0=10.0 ** rs.uniform(-20.0, -18.0, n),
                sizes=10.0 ** rs.uniform(14.0, 15.0, n))


def census_call(n):
    import sph_code_amd.compat as nsc
    s = seeded(n)
    cen = nsc.census(s["mass"], s["particle_type"], s["f_un"], None, s["velocities"], s["total_accel"], s["E_internal"])
    rows = [nsc.select_rows(s["mass"], s["particle_type"], t, T=s["T"], star_ages=s["star_ages"], f_un=s["f_un"]) for t in (0, 1, 2)]
    win = nsc.select_rows(s["mass"], s["particle_type"], 1, T=s["T"], window=nsc.AGB_WINDOW)
    return cen, rows, win


def adapt_call(n):
    import sph_code_amd.compat as nsc
    s = seeded(n)
    return nsc.adapt_sizes(s["neighbor"], s["densities"], s["densities_0"], s["sizes"], s["particle_type"], 3e14, 8.0, full=True)


FAMILIES = {"rad_cooling": cool_call, "supernova_destruction": dust_call, "chemisputtering_2": chem_call,
            "census_select_rows": census_call, "adapt_sizes": adapt_call}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_a_smaller_call_inside_grown_buffers_and_the_larger_one_again(family, monkeypatch):
    import sph_code_amd.compat as nsc
    call = FAMILIES[family]
    first = call(BIG)
    small = call(SMALL)
    third = call(BIG)
    assert same_bits(third, first), family
    monkeypatch.setattr(nsc, "_ctx", None)            # the next call creates a context of its own: nothing allocated yet
    monkeypatch.setattr(nsc, "_nb_held", None)
    try:
        fresh = call(SMALL)
    finally:
        own = nsc._ctx
        monkeypatch.undo()
        if own is not None:
            own.close()
    assert same_bits(small, fresh), family
    assert not same_bits(small, first)
