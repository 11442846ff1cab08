"""GPU tests (-m gpu): rad_columns, rad_transfer, Simulation.rad_transfer and rad_cooling on the transformed cases of
tests/rad_cool_frames.py - off-centre by up to 2^27 cloud sizes, at another unit of length, flattened, at N up to 20011 and
with one ray more than a workgroup holds.  tests/test_rad_cool_frames_cpu.py shows the cases sound.  Two references and no
new tolerance: the NumPy restatements on the SAME transformed inputs with the bounds they derive (rad_oracle, cool_oracle),
and, for shifts and scalings by powers of two, the GPU's own call on the untransformed case, bit for bit - both operations
read coordinates through differences alone, and those are exact on the snapped cases.

NOT YET RUN on an MI355X where this line stands (no GPU could be obtained); DESIGN 5.9 and 5.10 say what has run."""
import numpy as np
import pytest

import cool_fixture
import cool_oracle
import frames
import rad_cool_frames as rcf
import rad_fixture
import rad_oracle
from test_gpu_cool import check as cool_check, gpu as gpu_cooling
from test_gpu_rad import check as rad_check, gpu_transfer

pytestmark = pytest.mark.gpu

ROUT, COUT = rad_oracle.OUTPUTS, cool_oracle.OUTPUTS
AU = 149597870700.0


def gpu_columns(f, mode):
    import sph_code_amd.compat as nsc
    return dict(zip(("blocked", "star_distance"), nsc.rad_columns(*rcf.columns_args(f), mode=mode)))


_rad_base, _cool_base = {}, {}


def rad_base_call(name, mode, columns):
    """The GPU's own result on the snapped, untransformed case, once per (base, mode, entry point)."""
    key = (name, mode, columns)
    if key not in _rad_base:
        f = rcf.rad_base(name)[0]
        _rad_base[key] = gpu_columns(f, mode) if columns else gpu_transfer(rad_fixture.transfer_args(f), mode)
    return _rad_base[key]


def _bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.array_equal(got, want, equal_nan=True), \
        "%s: %d elements differ from the untransformed call" % (what, (got != want).sum())


@pytest.mark.parametrize("mode", rad_oracle.MODES)
@pytest.mark.parametrize("case", rcf.RAD_CASES, ids=rcf.case_id)
def test_rad_on_transformed_cases(case, mode):
    """All six outputs of compat.rad_transfer (scale_down: the two of compat.rad_columns) against the restatement of the same
    transformed inputs, the margin checked first; under a shift every output of both entry points equal to the call on the
    base bit for bit; under a scaling blocked s^2, star_distance / s and extinction s^2 equal to it."""
    name, frame = case
    f, meta = rcf.rad_case(*case)
    sc = meta["scale"]
    o = rcf.rad_reference(name, frame, mode)
    what = "%s %s" % (rcf.case_id(case), mode)
    assert o["margin"] > rad_fixture.MIN_MARGIN, (what, o["margin"])
    cols = gpu_columns(f, mode)
    for nm in ("blocked", "star_distance"):
        print(what, "rad_columns", nm, "worst |diff| / bound %.3g" % rad_oracle.worst_ratio(cols[nm], o[nm], o[nm + "_bound"]))
    for nm in ("blocked", "star_distance"):
        rad_oracle.assert_within(nm, cols[nm], o[nm], o[nm + "_bound"], what + " rad_columns")
    got = None
    if frame not in rcf.COLUMNS_ONLY:
        got = gpu_transfer(rad_fixture.transfer_args(f), mode)
        rad_check(got, o, o, what)
        _bits(got["blocked"], cols["blocked"], what + " blocked of the two entry points")
        assert np.count_nonzero(got["lf2"]) >= 0.5 * got["lf2"].size
    if frame in rcf.SHIFTS:
        bc, bt = rad_base_call(name, mode, True), rad_base_call(name, mode, False)
        for nm in ("blocked", "star_distance"):
            _bits(cols[nm], bc[nm], "%s rad_columns %s" % (what, nm))
        for nm in ROUT:
            _bits(got[nm], bt[nm], "%s %s" % (what, nm))
    if frame in rcf.SCALES:
        bc = rad_base_call(name, mode, True)
        _bits(cols["blocked"] * sc ** 2, bc["blocked"], what + " rad_columns blocked s^2")
        _bits(cols["star_distance"] / sc, bc["star_distance"], what + " rad_columns star_distance / s")
        if got is not None:
            bt = rad_base_call(name, mode, False)
            _bits(got["blocked"] * sc ** 2, bt["blocked"], what + " blocked s^2")
            _bits(got["star_distance"] / sc, bt["star_distance"], what + " star_distance / s")
            _bits(got["extinction"] * sc ** 2, bt["extinction"], what + " extinction s^2")


def _resident(state, pt, mass, clamp, src, lum, dst, cross, twin_too):
    """One step at a vanishing dt (the positions stay on their lattice), rad_transfer in both modes, one ordinary step;
    with twin_too a second Simulation that never calls rad_transfer takes the same steps."""
    import sph_code_amd.compat as nsc
    from sph_code_amd import _lib
    from sph_code_amd.sim import Simulation
    s = dict(state, particle_type=pt, mass=mass)
    ctxs, out = [], {}
    try:
        sims = []
        for _ in range(2 if twin_too else 1):
            ctx = _lib.Context()
            ctxs.append(ctx)
            ctx.set_constants(k_B=nsc.k, amu=nsc.amu, m_h=nsc.m_h, m_0=nsc.m_0, dt_0=nsc.dt_0, solar_luminosity=nsc.solar_luminosity,
                              c=nsc.c, pos_clamp=clamp)
            sims.append(Simulation(s, n_neigh=40, ctx=ctx))
        for sim in sims:
            sim.step(1, fixed_dt=1e-30)
        out["state"] = sims[0].download()
        for mode in rad_oracle.MODES:
            out[mode] = sims[0].rad_transfer(src, lum, dst, cross, 7.9e12, mode=mode, full=True)
        for sim in sims:
            sim.step(1)
        out["after"] = [sim.download() for sim in sims]
    finally:
        for ctx in ctxs:
            ctx.close()
    return out


def test_resident_state_far_from_the_origin():
    """Simulation.rad_transfer on the polytrope 2^27 cloud sizes from the origin: the bits of compat.rad_transfer on the
    downloaded state, the bits of the same call on the unshifted Simulation, and the loop's next step unchanged."""
    import sph_code_amd.compat as nsc
    s, _, meta = frames.frame_case("shift_27", "polytrope", 4097, 40)
    base, off = meta["base"], meta["offset"]
    n = s["points"].shape[0]
    rs = np.random.RandomState(19)
    pt, mass = np.array(s["particle_type"], dtype=np.float64), np.array(s["mass"], dtype=np.float64)
    stars = rs.choice(np.nonzero(pt == 0)[0], 5, replace=False)
    pt[stars] = 1.0
    mass[stars] *= 50.0
    cross = 10.0 ** rs.uniform(-25.0, -21.0, n)
    lum = 10.0 ** rs.uniform(0.0, 4.0, 5)
    targets = rs.choice(np.nonzero(pt != 1)[0], 21, replace=False)
    clamp = max(1e11 * AU, 4.0 * np.abs(s["points"]).max())
    src_b, dst_b = base["points"][stars].copy(), base["points"][targets].copy()          # snapped particle positions
    far = _resident(s, pt, mass, clamp, src_b + off, lum, dst_b + off, cross, True)
    near = _resident(base, pt, mass, clamp, src_b, lum, dst_b, cross, False)
    st = far["state"]
    assert np.array_equal(st["points"], s["points"]) and np.array_equal(near["state"]["points"], base["points"])
    for mode in rad_oracle.MODES:
        ref = nsc.rad_transfer(st["points"], pt, mass, st["sizes"], cross, s["mu_array"], src_b + off, lum, dst_b + off, 7.9e12,
                               mode=mode, full=True)
        for nm, a, b in zip(ROUT, far[mode], ref):
            assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), ("compat", mode, nm)
        assert np.count_nonzero(far[mode][3]) > 50 and np.all(np.isfinite(far[mode][0]))
        o = rad_oracle.transfer(st["points"], pt, mass, st["sizes"], cross, s["mu_array"], src_b + off, lum, dst_b + off, 7.9e12,
                                mode=mode)
        rad_check(dict(zip(ROUT, far[mode])), o, o, "resident shift_27 %s" % mode)
    # the search is frame-independent (test_gpu_frames), so the resident sizes are the same bits and so is every output
    assert np.array_equal(st["sizes"], near["state"]["sizes"]), \
        "resident sizes differ between the frames in %d rows" % (st["sizes"] != near["state"]["sizes"]).sum()
    for mode in rad_oracle.MODES:
        for nm, a, b in zip(ROUT, far[mode], near[mode]):
            assert np.array_equal(a, b, equal_nan=True), ("unshifted Simulation", mode, nm)
    a, b = far["after"]
    for key in ("points", "velocities", "total_accel", "E_internal", "T", "sizes", "densities", "num_densities", "visc_heat",
                "pressure"):
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    assert a["dt"] == b["dt"] and np.any(a["points"] != st["points"])


def cool_base_call(name):
    if name not in _cool_base:
        c = rcf.cool_base(name)[0]
        _cool_base[name] = gpu_cooling(cool_fixture.cloud_compat_args(c), c["d"])
    return _cool_base[name]


@pytest.mark.parametrize("case", rcf.COOL_CASES, ids=rcf.case_id)
def test_cooling_on_transformed_cases(case):
    """All four outputs of compat.rad_cooling, the row table included, against the restatement of the same transformed
    inputs; a second call gives the same bits (at N = 20011 the fill order of the reverse list really varies); under a
    shift every output equals the call on the base bit for bit."""
    name, frame = case
    c, meta = rcf.cool_case(*case)
    o = rcf.cool_reference(name, frame)
    what = rcf.case_id(case)
    got = gpu_cooling(cool_fixture.cloud_compat_args(c), c["d"])
    cool_check(got, o, o, what)
    gas = c["particle_type"] == 0
    assert np.count_nonzero(got["energy"][gas]) >= 0.5 * gas.sum()
    again = gpu_cooling(cool_fixture.cloud_compat_args(c), c["d"])
    for nm in COUT:
        assert np.array_equal(got[nm], again[nm], equal_nan=True), (what, nm, "second call")
    if frame in rcf.SHIFTS:
        base = cool_base_call(name)
        for nm in COUT:
            _bits(got[nm], base[nm], "%s %s" % (what, nm))
    if frame == "scale_up":
        assert got["rec_array"][5].max() < 0.5
    if frame == "half_capped":
        assert 0.2 <= float(np.mean(got["rec_array"][5] > 0.99)) <= 0.8
