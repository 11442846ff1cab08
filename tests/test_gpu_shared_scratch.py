"""GPU check of the scratch that rad_cooling, supernova_destruction and chemisputtering_2 share on a context: ONE
reverse-list buffer and ONE buffer for its segmented sort (sphx_rev_build, sphx_side.hip).  On one context the three
stages run in turn at a large and at a small shape, so that each meets the buffers once as a larger neighbour left them
and once smaller than the next stage needs; then the two resident phases, which run the same stages back to back.  Every
result is held to its stage's own comparison - the helpers of tests/test_gpu_cool.py, test_gpu_dust.py, test_gpu_chem.py,
test_gpu_phase.py and test_gpu_radphase.py, imported, with the seeds those tests use for the shapes."""
import pytest

import chem_fixture
import cool_fixture
import dust_fixture
import phase_fixture as pf
import test_gpu_chem as t_chem
import test_gpu_cool as t_cool
import test_gpu_dust as t_dust
import test_gpu_phase as t_phase
import test_gpu_radphase as t_rad

pytestmark = pytest.mark.gpu

BIG, SMALL = (2049, 40, 32), (257, 7, 15)


def cool_at(shape):
    n, K, _ = shape
    t_cool.check_cloud(cool_fixture.cloud(n, K, 100 + K), "cool n=%d K=%d" % (n, K))       # (test_seeded_clouds' seed)


def dust_at(shape):
    name = "n=%d K=%d S=%d" % shape
    t_dust.check_set(dust_fixture.cloud(*dict(dust_fixture.shape_specs(shape[1]))[name]), "dust " + name)


def chem_at(shape):
    name = "n=%d K=%d S=%d" % shape
    assert name in chem_fixture.SEEDS and name in dict(chem_fixture.shape_specs(shape[1]))
    t_chem.check(name)


def test_stages_and_phases_share_one_reverse_list(monkeypatch):
    import sph_code_amd.compat as nsc
    from sph_code_amd import _lib
    ctx = _lib.Context()
    ctx.set_constants(k_B=nsc.k, amu=nsc.amu, m_h=nsc.m_h, m_0=nsc.m_0, dt_0=nsc.dt_0, solar_luminosity=nsc.solar_luminosity, c=nsc.c)
    try:
        with monkeypatch.context() as m:                     # compat's calls run on ctx
            m.setattr(nsc, "_ctx", ctx)
            m.setattr(nsc, "_nb_held", None)
            for stage, shape in ((cool_at, BIG), (dust_at, SMALL), (chem_at, BIG), (cool_at, SMALL), (dust_at, BIG), (chem_at, SMALL)):
                stage(shape)
        # the resident phases on ctx after a step; their array routes on compat's own context, as in the phases' own tests
        spec = pf.SHAPES[0]
        assert spec == SMALL + (513,)
        sim, f = t_phase.prepared(spec, "loop", ctx=ctx)
        res, _ = t_phase.assert_equals_array_route(nsc, sim, f, "fraction", pf.shape_id(spec))
        assert res["chem_counts"]["rows"] > 0
        sim, f = t_rad.rad_prepared(spec, "loop", ctx=ctx)
        res, _, _ = t_rad.assert_equals_array_route(sim, f, "line")
        assert not res["skipped"]
    finally:
        ctx.close()
