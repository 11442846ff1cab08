"""Drop-in for the hot-path callables of the reference's physics module.

    import sph_code_amd.compat as nsc          # instead of: import navier_stokes_cleaned as nsc

Same names, positional signatures and return tuples as sph/navier_stokes_cleaned.py ("nsc"),
for the functions the driver sph/code_running.py ("drv") calls on the SPH inner loop:

    neighbors              nsc:541-552      drv:171,386,437
    hydro_update           nsc:556-671      drv:179
    density                nsc:693-702      drv:451
    dust_density           nsc:704-717      drv:452
    num_dens               nsc:744-753      drv:453
    net_impulse            nsc:719-742      drv:455
    del_pressure           nsc:755-774      drv:456
    artificial_viscosity   nsc:788-816      drv:458
    crossing_time          nsc:776-786      drv:222
    rad_cooling            nsc:1019-1176    drv:276
    supernova_destruction  nsc:1211-1263    drv:411
    chemisputtering_2      nsc:1265-1416    drv:405
    supernova_impulse      nsc:1192-1204    drv:351 (supernova_impulses: the loop drv:350-352)
    length_scale, adapt_sizes               drv:493-540 (the driver's own lines, no nsc function)
    luminosity_relation    nsc:174-200      (without its unused `imf` argument)
    census, advance_star_ages, supernova_schedule, run_outputs, select_rows
                                            drv:244, 339-342, 604, 616-622, 636, 656-664 (the driver's own lines)
    project_maps                            drv:563-597 (what the driver's scatter plot approximates: the projection)

and, under names of their own, the pieces rad_heating (nsc:893-1017) and the driver's radiative block (drv:247-316)
fall into: rad_setup, rad_transfer, stellar_spectrum, rad_ionise, rad_heat_bookkeeping, rad_cool_bookkeeping, and
rad_phase, which chains them with rad_cooling.

Hidden inputs are honoured the way the driver uses them: it assigns `nsc.d`, `nsc.d_0`,
`nsc.dt`, `nsc.dt_0` (drv:68-75,231) and the functions read the module attribute at call
time; each function also accepts `d=` explicitly.  Every function runs on the GPU through
libsphx.so (include/sphx.h); nothing here computes on the CPU.

Documented differences from the reference:
  * neighbors is exact (the eps=0 answer; eps=0.1 of nsc:544 is a permission, not a spec);
    element 1 of its return tuple (the cKDTree) is None.
  * hydro_update as committed raises IndexError at nsc:651 for every N > K; this module
    returns the result of the one shape-consistent reading (Pi summed over neighbours).
  * rows with missing neighbours (index == N) contribute zero instead of raising.
  * mass / f_un arrive as longdouble from the driver and are cast to float64.
"""
import itertools

import numpy as np

from . import _lib
from ._lib import dp, f64, i64, ip

# ---- constants read by the path (nsc:21-52) -----------------------------------------------
k = 1.380649e-23
amu = 1.66053906892e-27
AU = 149597870700.0
m_h = 1.0008 * amu
solar_mass = 1.989e30
solar_luminosity = 3.846e26
c = 299792458.0
m_0 = 10 ** 1.5 * solar_mass
year = 60. * 60. * 24. * 365.
dt_0 = year * 250000.
mu_specie = np.array([2.0158, 4.0026, 1.0079, 1.0074, 4.0021, 4.0016, 0.0005, 140.69, 60.08, 12.0107,
                      28.0855, 55.834, 100.39, 131.93, 40.096])
gamma = np.array([7. / 5, 5. / 3, 5. / 3, 5. / 3, 5. / 3, 5. / 3, 5. / 3, 15.6354113, 4.913, 1.0125,
                  2.364, 3.02, 10., 10., 10.])
f_u = np.array([.86, .14] + [0] * 13, dtype=float)
mineral_densities = np.array([1.e19] * 7 + [3320, 2260, 2266, 2329, 7870, 3250, 3250., 3166.])
mrn_constants = np.array([50e-10, 5000e-10])
sputtering_yields = np.array([0, 0, 0, 0, 0, 0, 0, 0.137, 0.295, 0.137, 0.295, 0.137, 0.137, 0.137, 0.137])   # nsc:45

# ---- driver-injected globals (drv:68-75); d has no default in the reference either ---------
d = None
d_0 = None
dt = dt_0

_ctx = None


def context():
    """The module's libsphx context (created on first use; GPU = $LOCAL_RANK or 0)."""
    global _ctx
    if _ctx is None:
        _ctx = _lib.Context()
        _ctx.set_constants(k_B=k, amu=amu, m_h=m_h, m_0=m_0, dt_0=dt_0, solar_luminosity=solar_luminosity, c=c)
    return _ctx


def _d(explicit):
    val = d if explicit is None else explicit
    if val is None:
        raise NameError("name 'd' is not defined (assign nsc.d as sph/code_running.py:68 does)")
    return float(val)


def _nk(neighbor):
    nb = i64(neighbor)
    if nb.ndim != 2:
        raise ValueError("neighbor must be (N, K)")
    return nb, nb.shape[0], nb.shape[1]


# The driver hands ONE neighbour array to eight calls per step (drv:451-458).  neighbors() returns it
# read-only; while that very object comes back, its device copy from the previous call is reused
# (neighbor = NULL in the C call) instead of 8 N K bytes crossing PCIe again.
_nb_held = None


def _with_nb(neighbor, nb, call):
    """call(pointer-or-None) -> rc, with the list of the previous call reused when it is this array."""
    global _nb_held
    c = context()
    reusable = isinstance(neighbor, np.ndarray) and neighbor is nb and not neighbor.flags.writeable
    if reusable and _nb_held is neighbor:
        rc = call(None)
        if rc != _lib.SPHX_E_STATE:              # (E_STATE: the context dropped the list: upload it)
            c.check(rc)
            return
    _nb_held = None
    c.check(call(ip(nb)))
    _nb_held = neighbor if reusable else None


def _mrn_limits(mrn_constants):
    lo, hi = float(mrn_constants[0]), float(mrn_constants[1])        # grain radii a_min, a_max
    return lo, hi


def grain_mass(mineral_densities=mineral_densities, mrn_constants=mrn_constants):
    """Mean grain mass per species for the MRN size law n(a) ~ a^-3.5 (the table nsc:76-79 builds):
    rho 4 pi/3 <a^3>, with <a^3> = (4/5) (a_max^0.5 - a_min^0.5) / (a_min^-2.5 - a_max^-2.5)."""
    lo, hi = _mrn_limits(mrn_constants)
    ratio = -(hi ** 0.5 - lo ** 0.5) / (hi ** -2.5 - lo ** -2.5)
    return mineral_densities * ratio * (4. / 5.) * 4 * np.pi / 3.


def sigma_effective(mineral_densities=mineral_densities, mrn_constants=mrn_constants, mu_specie=mu_specie):
    """Effective cross-section per species for the same size law (the table nsc:69-74 builds)."""
    lo, hi = _mrn_limits(mrn_constants)
    ratio = -(hi ** -0.5 - lo ** -0.5) / (hi ** 0.5 - lo ** 0.5)
    return mu_specie * amu / mineral_densities * (3. / 4.) * ratio


# ==============================================================================================
def neighbors(points, dist, N_NEIGH, eps=0.1):
    """nsc:541-552 -> (idx (N,K) int64, None, dist (N,K), nontriv (N,), new_sizes (N,))."""
    pts = f64(points)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError("points must be (N, 3)")
    n, K = pts.shape[0], int(N_NEIGH)
    c = context()
    idx = _lib.pinned.empty((n, K), np.int64)         # 8 N K bytes each: page-locked when large (4x the copy rate)
    dd = _lib.pinned.empty((n, K), np.float64)
    nontriv = np.empty(n, np.int64)
    h = np.empty(n, np.float64)
    bound = float(dist) if np.isfinite(dist) else 0.0
    global _nb_held
    _nb_held = None                                   # the search overwrites the context's list
    c.check(c.lib.sphx_neighbors(c.h, n, K, dp(pts), bound, float(eps), ip(idx), dp(dd), ip(nontriv), dp(h)))
    idx.setflags(write=False)                         # (np.copy(neighbor), drv:172, is writeable again)
    return idx, None, dd, nontriv, h


VISC_MODES = {"ref_axis0": 0, "pairwise": 1}


def visc_mode_code(visc_mode):
    """"ref_axis0" -> 0, "pairwise" -> 1 (include/sphx.h sphx_hydro_update); anything else: ValueError."""
    if not isinstance(visc_mode, str) or visc_mode not in VISC_MODES:
        raise ValueError("visc_mode must be 'ref_axis0' or 'pairwise', not %r" % (visc_mode,))
    return VISC_MODES[visc_mode]


def hydro_update(neighbor, points, mass, sizes, f_un, particle_type, T, mu_array, gamma_array, velocities,
                 clip_grad=False, visc_mode="ref_axis0"):
    """nsc:556-671 -> (hydro_accel (N,3), visc_accel (N,3), visc_heat (N,), density_calc (N,),
    num_density_calc (N,), f_un_neighbor (S,N), dust_density_calc (N,)).  clip_grad=True: the physics option
    of include/sphx.h sphx_set_clip_grad (not the reference's arithmetic).  visc_mode="pairwise": the per-pair
    pi_ik inside the viscous sum (include/sphx.h sphx_hydro_update); "ref_axis0" (the default) is the reference's."""
    mode = visc_mode_code(visc_mode)
    nb, n, K = _nk(neighbor)
    pts = f64(points, (n, 3)); vel = f64(velocities, (n, 3))
    m = f64(mass, (n,)); h = f64(sizes, (n,)); pt = f64(particle_type, (n,))
    Tt = f64(T, (n,)); mu = f64(mu_array, (n,)); gam = f64(gamma_array, (n,))
    fu = f64(f_un)
    if fu.ndim != 2 or fu.shape[0] != n:
        raise ValueError("f_un must be (N, S)")
    S = fu.shape[1]
    pe = _lib.pinned.empty                          # page-locked when large: faster device-to-host copies
    ha = pe((n, 3), np.float64); va = pe((n, 3), np.float64); vh = np.empty(n)
    rho = np.empty(n); nden = np.empty(n); F = pe((S, n), np.float64); rhod = np.empty(n)
    c = context()
    c.check(c.lib.sphx_set_clip_grad(c.h, 1 if clip_grad else 0))
    try:
        _with_nb(neighbor, nb, lambda nbp: c.lib.sphx_hydro_update(
            c.h, n, K, S, nbp, dp(pts), dp(m), dp(h), dp(fu), dp(pt), dp(Tt), dp(mu), dp(gam), dp(vel), mode,
            dp(ha), dp(va), dp(vh), dp(rho), dp(nden), dp(F), dp(rhod)))
    finally:
        c.lib.sphx_set_clip_grad(c.h, 0)
    return ha, va, vh, rho, nden, F, rhod


def density(points, mass, particle_type, neighbor, d=None):
    """nsc:693-702."""
    nb, n, K = _nk(neighbor)
    out = np.empty(n)
    c = context()
    pts, m, pt, dd = f64(points, (n, 3)), f64(mass, (n,)), f64(particle_type, (n,)), _d(d)
    _with_nb(neighbor, nb, lambda nbp: c.lib.sphx_density(c.h, n, K, dp(pts), dp(m), dp(pt), nbp, dd, dp(out)))
    return out


def dust_density(points, mass, neighbor, particle_type, sizes):
    """nsc:704-717."""
    nb, n, K = _nk(neighbor)
    out = np.empty(n)
    c = context()
    pts, m, pt, h = f64(points, (n, 3)), f64(mass, (n,)), f64(particle_type, (n,)), f64(sizes, (n,))
    _with_nb(neighbor, nb, lambda nbp: c.lib.sphx_dust_density(c.h, n, K, dp(pts), dp(m), nbp, dp(pt), dp(h), dp(out)))
    return out


def num_dens(mass, points, mu_array, neighbor, d=None):
    """nsc:744-753."""
    nb, n, K = _nk(neighbor)
    out = np.empty(n)
    c = context()
    m, pts, mu, dd = f64(mass, (n,)), f64(points, (n, 3)), f64(mu_array, (n,)), _d(d)
    _with_nb(neighbor, nb, lambda nbp: c.lib.sphx_num_dens(c.h, n, K, dp(m), dp(pts), dp(mu), nbp, dd, dp(out)))
    return out


def del_pressure(points, mass, particle_type, neighbor, E_internal, gamma_array, d=None):
    """nsc:755-774."""
    nb, n, K = _nk(neighbor)
    out = _lib.pinned.empty((n, 3), np.float64)
    c = context()
    pts, m, pt = f64(points, (n, 3)), f64(mass, (n,)), f64(particle_type, (n,))
    E, gam, dd = f64(E_internal, (n,)), f64(gamma_array, (n,)), _d(d)
    _with_nb(neighbor, nb, lambda nbp: c.lib.sphx_del_pressure(c.h, n, K, dp(pts), dp(m), dp(pt), nbp, dp(E),
                                                               dp(gam), dd, dp(out)))
    return out


def artificial_viscosity(neighbor, points, particle_type, sizes, mass, densities, velocities, T,
                         gamma_array, mu_array, d=None):
    """nsc:788-816 -> (visc_accel (N,3), visc_heat (N,))."""
    nb, n, K = _nk(neighbor)
    acc = _lib.pinned.empty((n, 3), np.float64); heat = np.empty(n)
    c = context()
    pts, pt, h, m = f64(points, (n, 3)), f64(particle_type, (n,)), f64(sizes, (n,)), f64(mass, (n,))
    rho, vel, Tt = f64(densities, (n,)), f64(velocities, (n, 3)), f64(T, (n,))
    gam, mu, dd = f64(gamma_array, (n,)), f64(mu_array, (n,)), _d(d)
    _with_nb(neighbor, nb, lambda nbp: c.lib.sphx_artificial_viscosity(
        c.h, n, K, nbp, dp(pts), dp(pt), dp(h), dp(m), dp(rho), dp(vel), dp(Tt), dp(gam), dp(mu), dd,
        dp(acc), dp(heat)))
    return acc, heat


def crossing_time(neighbor, velocities, sizes, particle_type):
    """nsc:776-786 -> scalar."""
    nb, n, K = _nk(neighbor)
    out = np.empty(1)
    c = context()
    c.set_constants(dt_0=float(dt_0))
    vel, h, pt = f64(velocities, (n, 3)), f64(sizes, (n,)), f64(particle_type, (n,))
    _with_nb(neighbor, nb, lambda nbp: c.lib.sphx_crossing_time(c.h, n, K, nbp, dp(vel), dp(h), dp(pt), dp(out)))
    return float(out[0])


def net_impulse(points, mass, sizes, velocities, particle_type, neighbor, f_un):
    """nsc:719-742 -> (accel_onto (N,3), accel_reaction (N,3))."""
    nb, n, K = _nk(neighbor)
    fu = f64(f_un)
    meff = grain_mass(mineral_densities, mrn_constants)
    seff = sigma_effective(mineral_densities, mrn_constants, mu_specie)
    mgm = np.ascontiguousarray(np.sum(meff * fu, axis=1))        # nsc:725 (per particle)
    mcs = np.ascontiguousarray(np.sum(seff * fu, axis=1))        # nsc:726
    onto = _lib.pinned.empty((n, 3), np.float64); react = _lib.pinned.empty((n, 3), np.float64)
    c = context()
    pts, m, h = f64(points, (n, 3)), f64(mass, (n,)), f64(sizes, (n,))
    vel, pt = f64(velocities, (n, 3)), f64(particle_type, (n,))
    _with_nb(neighbor, nb, lambda nbp: c.lib.sphx_net_impulse(c.h, n, K, dp(pts), dp(m), dp(h), dp(vel), dp(pt),
                                                              nbp, dp(mgm), dp(mcs), dp(onto), dp(react)))
    return onto, react


def grav_force_direct(mass, points, sizes, G=6.67430e-11):
    """Softened direct-sum self-gravity, (n,3): G m_j (x_j - x_i) / (|x_j - x_i|^2 + eps^2)^(3/2) over all j,
    eps = median(sizes) - the call shape of nsc.grav_force_calculation_new(mass, points, sizes) (nsc:252,
    softening nsc:358,385).  NOT that function's result: the reference sums a few kd-tree monopoles and
    cannot be run for comparison; this is the exact sum such a tree approximates."""
    c = context()
    pts = np.ascontiguousarray(points, dtype=np.float64)
    n = pts.shape[0]
    m = np.ascontiguousarray(mass, dtype=np.float64)
    h = np.ascontiguousarray(sizes, dtype=np.float64)
    out = np.empty((n, 3))
    dp = lambda a: a.ctypes.data_as(_lib.c_double_p)
    c.check(c.lib.sphx_gravity_direct(c.h, n, dp(m), dp(pts), dp(h), 0.0, float(G), dp(out)))
    return out


def grav_force_tree(mass, points, sizes, G=6.67430e-11, ws=1, order=2):
    """The sum of grav_force_direct by multipoles of a cell pyramid (include/sphx.h: sphx_gravity_tree), O(N).
    order 2 (cells carry their second moments; the default) gives ~0.1 % rms force error at ws = 1 and
    ~0.01 % at ws = 2; order 1 (monopoles) ~1 % and ~0.2 %."""
    c = context()
    pts = np.ascontiguousarray(points, dtype=np.float64)
    n = pts.shape[0]
    m = np.ascontiguousarray(mass, dtype=np.float64)
    h = np.ascontiguousarray(sizes, dtype=np.float64)
    out = np.empty((n, 3))
    dp = lambda a: a.ctypes.data_as(_lib.c_double_p)
    c.check(c.lib.sphx_set_gravity_order(c.h, int(order)))       # 2: cells carry quadrupoles too
    try:
        c.check(c.lib.sphx_gravity_tree(c.h, n, dp(m), dp(pts), dp(h), 0.0, float(G), int(ws), 40, dp(out)))
    finally:
        c.lib.sphx_set_gravity_order(c.h, 2)
    return out


GRAVPOT_STAGES = ("upload", "build", "sum", "download")


def _gravpot_args(mass, points, sizes, return_accel):
    pts = np.ascontiguousarray(points, dtype=np.float64)
    n = pts.shape[0]
    return (n, np.ascontiguousarray(mass, dtype=np.float64), pts, np.ascontiguousarray(sizes, dtype=np.float64),
            np.empty((n, 3)) if return_accel else None, np.empty(n))


def grav_potential_direct(mass, points, sizes, G=6.67430e-11, return_accel=False):
    """The potential of grav_force_direct's sum, (n,) in J/kg: phi_i = -G sum_{j != i} m_j / sqrt(|x_j - x_i|^2 + eps^2),
    eps = median(sizes); row i is left out of its own sum by index (include/sphx.h: sphx_gravity_direct_pot).
    U = 0.5 * np.sum(mass * phi).  return_accel: -> (phi, accel), accel the bits of grav_force_direct."""
    c = context()
    n, m, pts, h, acc, phi = _gravpot_args(mass, points, sizes, return_accel)
    c.check(c.lib.sphx_gravity_direct_pot(c.h, n, dp(m), dp(pts), dp(h), 0.0, float(G), dp(acc), dp(phi)))
    return (phi, acc) if return_accel else phi


def grav_potential_tree(mass, points, sizes, G=6.67430e-11, ws=1, order=2, return_accel=False):
    """The potential of grav_force_tree's sum by the same walk over the same cells (include/sphx.h: sphx_gravity_tree_pot):
    a cell of order 2 adds -G [M / s + 3/2 (r.S.r) / s^5 - 1/2 tr S / s^3], of order 1 -G M / s.  return_accel:
    -> (phi, accel), accel the bits of grav_force_tree."""
    c = context()
    n, m, pts, h, acc, phi = _gravpot_args(mass, points, sizes, return_accel)
    c.check(c.lib.sphx_set_gravity_order(c.h, int(order)))
    try:
        c.check(c.lib.sphx_gravity_tree_pot(c.h, n, dp(m), dp(pts), dp(h), 0.0, float(G), int(ws), dp(acc), dp(phi)))
    finally:
        c.lib.sphx_set_gravity_order(c.h, 2)
    return (phi, acc) if return_accel else phi


def gravpot_last_timing():
    """Device time of the last grav_potential_* call of this module from HIP events -> dict of ms (GRAVPOT_STAGES)."""
    return _last_timing("sphx_gravpot_last_timing", GRAVPOT_STAGES)


def grav_force_tree_parts(mass, points, sizes, part_of, G=6.67430e-11, ws=1, order=2, return_counts=False):
    """grav_force_tree over a cloud held in parts (domains of an out-of-core run, ranks of a decomposed one): every part
    builds the pyramid over its own particles and sums its own field; to each other part it sends its mass as a flat
    list - the coarsest cells that stand ws cell edges clear of that part's bounding box as multipole records, the rest
    as particles - and every part adds the lists it receives (include/sphx.h: sphx_gravity_tree_parts).  part_of (n,)
    holds labels 0 .. max; a label nobody carries is an empty part.  ws = 0 sends everything as particles: the exact sum
    of grav_force_direct.  return_counts: also the (parts, parts, 2) array of cells and particles part a sent to part b."""
    c = context()
    pts = np.ascontiguousarray(points, dtype=np.float64)
    n = pts.shape[0]
    m = np.ascontiguousarray(mass, dtype=np.float64)
    h = np.ascontiguousarray(sizes, dtype=np.float64)
    lab = np.ascontiguousarray(part_of, dtype=np.int32)
    if lab.shape != (n,):
        raise ValueError("part_of must have one label per particle")
    nparts = int(lab.max()) + 1 if n else 1
    out = np.empty((n, 3))
    counts = np.zeros((nparts, nparts, 2), dtype=np.int64)
    dp = lambda a: a.ctypes.data_as(_lib.c_double_p)
    c.check(c.lib.sphx_set_gravity_order(c.h, int(order)))
    try:
        c.check(c.lib.sphx_gravity_tree_parts(c.h, n, dp(m), dp(pts), dp(h), 0.0, float(G), int(ws), 40, nparts,
                                              lab.ctypes.data_as(_lib.c_int32_p), dp(out),
                                              counts.ctypes.data_as(_lib.c_int64_p)))
    finally:
        c.lib.sphx_set_gravity_order(c.h, 2)
    return (out, counts) if return_counts else out


# ==============================================================================================
# The driver's inline integrator statements (the reference has no function for them)
# ==============================================================================================
MAX_AGE = 3e7 * year            # drv:78


def timestep(ct, first):
    """drv:223-229: dt from the crossing time (`first` = the driver's `age == 0`)."""
    c = context()
    c.set_constants(dt_0=float(dt_0), max_age=float(MAX_AGE))
    cts = np.array([ct], dtype=np.float64)
    fl = np.array([1 if first else 0], dtype=np.int32)
    out = np.empty(1)
    c.check(c.lib.sphx_dt_rule(c.h, 1, dp(cts), fl.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int32)), dp(out)))
    return float(out[0])


def clamp_state(points, velocities):
    """drv:233-238 -> (points, velocities) clamped to |x| <= 1e11 AU and nan_to_num'ed (new arrays)."""
    p = np.array(points, dtype=np.float64, order="C")
    v = np.array(velocities, dtype=np.float64, order="C")
    c = context()
    c.check(c.lib.sphx_clamp_arrays(c.h, p.shape[0], dp(p), dp(v)))
    return p, v


def leapfrog(points, velocities, total_accel, E_internal, mass, mu_array, gamma_array, particle_type, delp,
             densities, av, dt, grav_accel=None, dust_densities=None, viscous_drag=None):
    """drv:460-491 with the driver's variable names: `av` = nsc.artificial_viscosity's (accel, heat),
    `viscous_drag` = nsc.net_impulse's (onto_gas, reaction) or None, `total_accel` = the previous step's (None or a
    different shape: dv = a dt, drv:484-485).  -> (points, velocities, total_accel, E_internal, T), new arrays."""
    p = np.array(points, dtype=np.float64, order="C")
    n = p.shape[0]
    v = np.array(velocities, dtype=np.float64, order="C")
    E = np.array(E_internal, dtype=np.float64, order="C")
    old = None if total_accel is None or np.shape(total_accel) != (n, 3) else f64(total_accel, (n, 3))
    tot = np.empty((n, 3)); T = np.empty(n)
    m, mu, gam, pt = f64(mass, (n,)), f64(mu_array, (n,)), f64(gamma_array, (n,)), f64(particle_type, (n,))
    G, rho = f64(delp, (n, 3)), f64(densities, (n,))
    ava, avh = f64(av[0], (n, 3)), f64(av[1], (n,))
    gr = None if grav_accel is None else f64(grav_accel, (n, 3))
    rd = None if dust_densities is None else f64(dust_densities, (n,))
    don = dre = None
    if viscous_drag is not None:
        don, dre = f64(viscous_drag[0], (n, 3)), f64(viscous_drag[1], (n, 3))
    c = context()
    c.set_constants(k_B=k, m_h=m_h)
    c.check(c.lib.sphx_leapfrog(c.h, n, dp(p), dp(v), dp(tot), dp(old), dp(E), dp(T), dp(m), dp(mu), dp(gam), dp(pt),
                                dp(gr), dp(G), dp(rho), dp(rd), dp(don), dp(dre), dp(ava), dp(avh), float(dt)))
    return p, v, tot, E, T


# ==============================================================================================
# Fields at arbitrary points (nsc:1418-1529): the "very high-resolution graphs for publication"
# ==============================================================================================
ARB_FIELDS = ("density", "dust_density", "temperature", "dust_temperature", "photoionization")


class _ArbRow:
    """handle[j]: stands for the j-th ball where only its length is asked for (nsc:1432: len(narb[j]) > 1)."""
    __slots__ = ("n",)

    def __init__(self, n):
        self.n = int(n)

    def __len__(self):
        return self.n


class ArbBall:
    """What neighbors_arb returns instead of nsc:1422-1426's list of lists: the particle positions, the query points
    and the ball radius R = max(sizes).  The ball itself is never stored - the *_arb functions given a handle evaluate
    the exact (eps = 0) ball on the device's cell grid.  The first call on a handle builds the particles' cell list and
    sorts the query points; the library keeps both on the device under the handle's id, so the calls that follow on the
    same handle (the reference calls its five functions one after the other) upload the per-particle scalars alone and
    go straight to the sums (include/sphx.h sphx_arb_fields, ball_id).  One handle is held at a time: alternating
    between two handles rebuilds.  The handle is for the positions and points it was made with: the functions refuse
    other ones, and arrays changed in place afterwards need a new handle.  (Pass the very arrays the handle was made
    with: they are recognised by identity.  An equal copy is compared element by element, an O(N + M) pass over
    host memory on every call.)
    len(handle) == M; len(handle[j]) is the exact member count (counted for all points on first use, no sums formed).
    Counting is a call of its own with its own cell size (it knows no masses), so it replaces the ball the library
    holds: ask for the counts before or after the five field calls, not between them - or take "count" from
    arb_fields(..., with_stats=True), which fills the handle's counts on the way."""
    _ids = itertools.count(1)

    def __init__(self, points, arb_points, radius):
        self.points = f64(points)
        self.arb_points = f64(arb_points).reshape(-1, 3)
        self.radius = float(radius)
        self.ball_id = next(ArbBall._ids)
        self._counts = None

    def __len__(self):
        return self.arb_points.shape[0]

    def _check(self, pts, q):
        for mine, theirs, what in ((self.points, pts, "points"), (self.arb_points, q, "arb_points")):
            if mine is not theirs and not (mine.shape == theirs.shape and np.array_equal(mine, theirs, equal_nan=True)):
                raise ValueError("%s are not the ones this neighbors_arb handle was made for" % what)

    @property
    def counts(self):
        if self._counts is None:
            n, m = self.points.shape[0], len(self)
            cnt = np.zeros(m, np.int64)
            cand = np.zeros(1, np.int64)
            ones, zeros = np.ones(n), np.zeros(n)          # (required arguments; only the cell size is drawn from them)
            c = context()
            c.check(c.lib.sphx_arb_fields(c.h, n, dp(self.points), dp(ones), dp(zeros), None, None, None, None,
                                          self.radius / 2.0, m, dp(self.arb_points), self.radius, None, None, None, None,
                                          None, ip(cnt), ip(cand), 0))
            self._counts = cnt
        return self._counts

    def __getitem__(self, j):
        return _ArbRow(self.counts[j])


def neighbors_arb(points, arb_points, sizes):
    """nsc:1422-1426 -> ArbBall (the exact ball of radius max(sizes); the reference asks cKDTree for eps = 0.1)."""
    pts = f64(points)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError("points must be (N, 3)")
    return ArbBall(pts, arb_points, np.max(f64(sizes)))


def _arb_csr(narb, m):
    """any sequence of index sequences (what nsc.neighbors_arb returns) -> CSR (row_start (m+1), members) int64."""
    if len(narb) != m:
        raise ValueError("narb has %d rows for %d arb_points" % (len(narb), m))
    lens = np.fromiter((len(r) for r in narb), dtype=np.int64, count=m)
    row_start = np.zeros(m + 1, np.int64)
    np.cumsum(lens, out=row_start[1:])
    members = np.empty(int(row_start[-1]), np.int64)
    for j, r in enumerate(narb):
        members[row_start[j]:row_start[j + 1]] = r
    return row_start, members


def arb_fields(points, arb_points, mass, particle_type, narb, sizes=None, T=None, N_PART=None, photoionization=None,
               d=None, fields=ARB_FIELDS, with_stats=False):
    """Every requested field of nsc:1428-1527 in ONE pass over the balls -> dict of (M,) arrays (what the five *_arb
    functions below call with one field each).  narb: an ArbBall (grid form, exact ball) or any sequence of index
    sequences (list form, honoured as given).  A field whose inputs are missing raises ValueError.
    with_stats: the dict also carries "count" (M,) int64 and "candidates" (pair evaluations)."""
    pts = f64(points)
    n = pts.shape[0]
    q = f64(arb_points).reshape(-1, 3)
    m = q.shape[0]
    opt = lambda a: None if a is None else f64(a, (n,))
    ms, pt, sz, Tt, npart, val = f64(mass, (n,)), f64(particle_type, (n,)), opt(sizes), opt(T), opt(N_PART), opt(photoionization)
    need = {"density": (), "dust_density": (sz,), "temperature": (Tt,), "dust_temperature": (sz, Tt),
            "photoionization": (npart, val)}
    out = {}
    for f in fields:
        if f not in need:
            raise ValueError("unknown field %r (one of %s)" % (f, ", ".join(ARB_FIELDS)))
        if any(a is None for a in need[f]):
            raise ValueError("field %r needs inputs that were not given" % f)
        out[f] = np.zeros(m)
    ptrs = [dp(out.get(f)) for f in ARB_FIELDS]
    cnt = np.zeros(m, np.int64) if with_stats else None
    cand = np.zeros(1, np.int64)
    c = context()
    if isinstance(narb, ArbBall):
        narb._check(pts, q)
        c.check(c.lib.sphx_arb_fields(c.h, n, dp(pts), dp(ms), dp(pt), dp(sz), dp(Tt), dp(npart), dp(val), _d(d), m, dp(q),
                                      narb.radius, *ptrs, ip(cnt), ip(cand), narb.ball_id))
        if with_stats and narb._counts is None:
            narb._counts = cnt.copy()
    else:
        row_start, members = _arb_csr(narb, m)
        c.check(c.lib.sphx_arb_fields_list(c.h, n, dp(pts), dp(ms), dp(pt), dp(sz), dp(Tt), dp(npart), dp(val), _d(d), m,
                                           dp(q), ip(row_start), ip(members), *ptrs, ip(cnt), ip(cand)))
    if with_stats:
        out["count"] = cnt
        out["candidates"] = int(cand[0])
    return out


def density_arb(points, arb_points, mass, particle_type, narb, d=None):
    """nsc:1428-1443."""
    return arb_fields(points, arb_points, mass, particle_type, narb, d=d, fields=("density",))["density"]


def dust_density_arb(points, arb_points, mass, particle_type, sizes, narb, d=None):
    """nsc:1445-1461."""
    return arb_fields(points, arb_points, mass, particle_type, narb, sizes=sizes, d=d,
                      fields=("dust_density",))["dust_density"]


def temperature_arb(points, arb_points, mass, particle_type, T, narb, d=None):
    """nsc:1463-1486."""
    return arb_fields(points, arb_points, mass, particle_type, narb, T=T, d=d, fields=("temperature",))["temperature"]


def dust_temperature_arb(points, arb_points, mass, particle_type, sizes, T, narb, d=None):
    """nsc:1488-1508."""
    return arb_fields(points, arb_points, mass, particle_type, narb, sizes=sizes, T=T, d=d,
                      fields=("dust_temperature",))["dust_temperature"]


def photoionization_arb(points, arb_points, mass, N_PART, photoionization, particle_type, narb, d=None):
    """nsc:1510-1527."""
    return arb_fields(points, arb_points, mass, particle_type, narb, N_PART=N_PART, photoionization=photoionization,
                      d=d, fields=("photoionization",))["photoionization"]


def _last_timing(getter, names):
    """The stage times (ms) a family's sphx_*_last_timing reports for the module context, under `names`."""
    out = np.zeros(len(names))
    c = context()
    c.check(getattr(c.lib, getter)(c.h, dp(out)))
    return dict(zip(names, out.tolist()))


def arb_last_timing():
    """Device time of the last *_arb / arb_fields call of this module, from HIP events (include/sphx.h
    sphx_arb_last_timing) -> dict of ms: upload, build, kernels, download."""
    return _last_timing("sphx_arb_last_timing", ("upload", "build", "kernels", "download"))


# ==============================================================================================
# Radiative transfer: the geometry and the deposition of rad_heating (nsc:922-965)
# ==============================================================================================
RAD_MODES = {"line": 0, "segment": 1}


def rad_mode_code(mode):
    """"line" -> 0, "segment" -> 1 (include/sphx.h SPHX_RAD_LINE / SPHX_RAD_SEGMENT); anything else: ValueError."""
    if not isinstance(mode, str) or mode not in RAD_MODES:
        raise ValueError("mode must be 'line' or 'segment', not %r" % (mode,))
    return RAD_MODES[mode]


def _pts3(a, what):
    out = f64(a)
    if out.size == 0:
        return np.zeros((0, 3))
    if out.ndim != 2 or out.shape[1] != 3:
        raise ValueError("%s must be (M, 3)" % what)
    return out


def rad_columns(positions, sizes, masses, mu_array, cross_array, sources, targets, mode="line"):
    """The columns of nsc:922-931 between any two point sets -> (blocked, star_distance), each (n_src, n_dst):
    blocked[s,q] = sum over the particles within their own h of the line through sources[s] and targets[q] of
    C2 h^-2 cross m / (mu amu), C2 = 3 pi / 80; star_distance[s,q] = |targets[q] - sources[s]|.  mode="segment" (not the
    reference's reading) counts only particles whose foot point lies between the two (include/sphx.h)."""
    code = rad_mode_code(mode)
    pts = _pts3(positions, "positions")
    n = pts.shape[0]
    src, dst = _pts3(sources, "sources"), _pts3(targets, "targets")
    h, m, mu, cr = f64(sizes, (n,)), f64(masses, (n,)), f64(mu_array, (n,)), f64(cross_array, (n,))
    blocked = np.zeros((src.shape[0], dst.shape[0])); sd = np.zeros((src.shape[0], dst.shape[0]))
    c_ = context()
    c_.check(c_.lib.sphx_rad_columns(c_.h, n, dp(pts), dp(h), dp(m), dp(mu), dp(cr), src.shape[0], dp(src), dst.shape[0],
                                     dp(dst), code, dp(blocked), dp(sd)))
    return blocked, sd


def _rad_outputs(n_gas, n_src, n_dst, full):
    lf2 = np.zeros(n_gas); mom = np.zeros((n_gas, 3)); ext = np.zeros(n_gas)
    if not full:
        return [lf2, mom, ext], [None, None, None]
    return [lf2, mom, ext], [np.zeros((n_src, n_dst)), np.zeros((n_src, n_dst)), np.zeros((n_src, n_gas))]


def rad_transfer(positions, ptypes, masses, sizes, cross_array, mu_array, sources, luminosities, targets, dt, mode="line",
                 full=False):
    """Lines 922-965 of nsc.rad_heating (nsc:893), with its argument names: the columns between the selected stars and
    the sampled gas particles, their spread over every non-star particle, and the energy and momentum deposited
    -> (lf2 (G,), momentum (G,3), extinction (G,)) over the G particles with ptypes != 1, as rad_heating returns them;
    full=True: also blocked, star_distance (n_src, n_dst) and lum_factor (n_src, G).
    What stays with the caller: the star selection and `luminosities` of nsc:897-921 (sources = the reference's rs2,
    targets = its rg2) and the composition chemistry of nsc:967-1017.  ValueError when no particle has ptypes == 0
    (the reference raises there too).  mode="segment": include/sphx.h, not the reference's reading."""
    code = rad_mode_code(mode)
    pts = _pts3(positions, "positions")
    n = pts.shape[0]
    src, dst = _pts3(sources, "sources"), _pts3(targets, "targets")
    pt, m, h = f64(ptypes, (n,)), f64(masses, (n,)), f64(sizes, (n,))
    cr, mu = f64(cross_array, (n,)), f64(mu_array, (n,))
    L = f64(luminosities).reshape(-1)
    if L.shape[0] != src.shape[0]:
        raise ValueError("luminosities must have one entry per source")
    main, extra = _rad_outputs(int(np.count_nonzero(pt != 1)), src.shape[0], dst.shape[0], full)
    c_ = context()
    c_.set_constants(amu=amu, solar_luminosity=solar_luminosity, c=c)
    c_.check(c_.lib.sphx_rad_transfer(c_.h, n, dp(pts), dp(pt), dp(m), dp(h), dp(cr), dp(mu), src.shape[0], dp(src), dp(L),
                                      dst.shape[0], dp(dst), float(dt), code, *[dp(a) for a in main + extra]))
    return tuple(main + extra) if full else tuple(main)


def rad_last_timing():
    """Device time of the last rad_columns / rad_transfer call of this module, from HIP events (include/sphx.h
    sphx_rad_last_timing) -> dict of ms: upload, columns, deposit, download."""
    return _last_timing("sphx_rad_last_timing", ("upload", "columns", "deposit", "download"))


# ==============================================================================================
# Radiative cooling: rad_cooling (nsc:1019-1176)
# ==============================================================================================
def rad_cooling(positions, particle_type, masses, sizes, cross_array, f_un, neighbor, mu_array, T, dt, d=None, full=False):
    """nsc:1019-1176 -> (final_comp (N,S), energy (N,), rec_array (S,N)); full=True appends the (N,6) table of the rows'
    scalars (f_Hn, f_H, f_He, f_e, E_H, E_He).  sizes and cross_array are accepted and never read, as in the reference.
    The two np.min calls of nsc:1089, 1094 (a TypeError as committed) are read as np.minimum; the other quirks are kept
    (include/sphx.h, sphx_rad_cooling).  f_un passes through nan_to_num on ingest, as nsc:1023 does."""
    nb, n, K = _nk(neighbor)
    pts, pt, m = f64(positions, (n, 3)), f64(particle_type, (n,)), f64(masses, (n,))
    mu, temp, dd = f64(mu_array, (n,)), f64(T, (n,)), _d(d)
    fun = np.nan_to_num(f64(f_un))
    if fun.ndim != 2 or fun.shape[0] != n:
        raise ValueError("f_un must be (N, S)")
    S = fun.shape[1]
    final = np.empty((n, S)); energy = np.empty(n); rec = np.empty((S, n))
    table = np.empty((n, 6)) if full else None
    c_ = context()
    c_.set_constants(k_B=k, m_h=m_h, m_0=m_0)
    c_.check(c_.lib.sphx_rad_cooling(c_.h, n, K, S, dp(pts), dp(pt), dp(m), dp(fun), ip(nb), dp(mu), dp(temp), float(dt), dd,
                                     dp(final), dp(energy), dp(rec), dp(table)))
    return (final, energy, rec, table) if full else (final, energy, rec)


def cool_last_timing():
    """Device time of the last rad_cooling call of this module, from HIP events (include/sphx.h sphx_cool_last_timing)
    -> dict of ms: upload, rows, gather, download."""
    return _last_timing("sphx_cool_last_timing", ("upload", "rows", "gather", "download"))


# ==============================================================================================
# Shock sputtering of dust: supernova_destruction (nsc:1211-1263)
# ==============================================================================================
critical_density = 1000 * amu * 10 ** 6                                         # nsc:49
crit_mass = 0.0001 * solar_mass                                                 # nsc:50 (the driver rescales it by raise_factor)
DUST_KNOTS_V = (0., 50., 75., 100., 125., 150., 175., 200.)                     # nsc:148-150, km/s
DUST_KNOTS_C = (0., 0.01, 0.04, 0.10, 0.18, 0.17, 0.18, 0.23)
DUST_KNOTS_SI = (0., 0.02, 0.09, 0.23, 0.41, 0.40, 0.42, 0.40)
DUST_CURVES = (0, 0, 0, 0, 0, 0, 1, 2, 1, 2, 1, 1, 1, 0)                        # nsc:159: 0 none, 1 carbon, 2 silicon
DUST_GUARDS = {"count": 0, "fraction": 1}
DUST_COUNTS = ("lost", "accepted", "rejected", "rejected_by_accumulation", "capped")


def dust_species_curve(S, species_curve=None):
    """The selector of length S as int32: the reference's 14-entry tuple padded with 0 ("none") by default (SURVEY
    Appendix B Q13); a given one must have S entries of 0, 1 or 2."""
    if species_curve is None:
        if S < len(DUST_CURVES):
            return np.array(DUST_CURVES[:S], dtype=np.int32)
        return np.array(DUST_CURVES + (0,) * (S - len(DUST_CURVES)), dtype=np.int32)
    sc = np.ascontiguousarray(species_curve, dtype=np.int32)
    if sc.shape != (S,) or np.any(sc < 0) or np.any(sc > 2):
        raise ValueError("species_curve must hold S = %d entries of 0, 1 or 2" % S)
    return sc


def supernova_destruction(points, velocities, neighbor, mass, f_un, mu_array, sizes, densities, particle_type,
                          crit_mass=None, critical_density=None, species_curve=None, guard="count", full=False):
    """nsc:1211-1263 -> (frac_destruction (N,S), frac_reuptake (N,S)); full=True appends a dict of the regime counts
    (DUST_COUNTS).  crit_mass and critical_density default to the module's values, read at call time (the driver
    rescales crit_mass).  species_curve: per species 0 none, 1 the carbon curve, 2 the silicon curve; by default the
    reference's 14-entry tuple padded with "none" to S - as committed that tuple is one entry short of the 15 species
    and the function raises.  guard="count" is the reference's comparison of an atom count with 1; guard="fraction" (not
    the reference's) keeps a species' accumulated loss below the particle's atom count.  include/sphx.h,
    sphx_supernova_destruction, lists the quirks kept."""
    if not isinstance(guard, str) or guard not in DUST_GUARDS:
        raise ValueError("guard must be 'count' or 'fraction', not %r" % (guard,))
    nb, n, K = _nk(neighbor)
    pts, vel = f64(points, (n, 3)), f64(velocities, (n, 3))
    m, mu, h = f64(mass, (n,)), f64(mu_array, (n,)), f64(sizes, (n,))
    dens, pt = f64(densities, (n,)), f64(particle_type, (n,))
    fun = f64(f_un)
    if fun.ndim != 2 or fun.shape[0] != n:
        raise ValueError("f_un must be (N, S)")
    S = fun.shape[1]
    sc = dust_species_curve(S, species_curve)
    g = globals()
    cm = float(g["crit_mass"] if crit_mass is None else crit_mass)
    cd = float(g["critical_density"] if critical_density is None else critical_density)
    kv, kc, ks = (np.array(a, dtype=np.float64) for a in (DUST_KNOTS_V, DUST_KNOTS_C, DUST_KNOTS_SI))
    destr = np.empty((n, S)); reup = np.empty((n, S))
    counts = np.zeros(len(DUST_COUNTS), dtype=np.int64) if full else None
    c_ = context()
    c_.set_constants(amu=amu)
    c_.check(c_.lib.sphx_supernova_destruction(c_.h, n, K, S, dp(pts), dp(vel), ip(nb), dp(m), dp(fun), dp(mu), dp(h), dp(dens),
                                               dp(pt), cm, cd, sc.ctypes.data_as(_lib.c_int32_p), dp(kv), dp(kc), dp(ks),
                                               DUST_GUARDS[guard], dp(destr), dp(reup), ip(counts)))
    if full:
        return destr, reup, dict(zip(DUST_COUNTS, (int(v) for v in counts)))
    return destr, reup


def dust_last_timing():
    """Device time of the last supernova_destruction call of this module, from HIP events (include/sphx.h
    sphx_dust_last_timing) -> dict of ms: upload, reverse, dust, rows."""
    return _last_timing("sphx_dust_last_timing", ("upload", "reverse", "dust", "rows"))


# ==============================================================================================
# The kick of an exploding star on the gas around it: supernova_impulse (nsc:1192-1204)
# ==============================================================================================
supernova_energy = 1e44                                                         # nsc:35, J
mass_displaced = 194.28 * solar_mass                                            # nsc:1193
SN_KICK_FRACTION = 0.736                                                        # nsc:1200
SN_COUNTS = ("candidates", "lds_sorts", "global_sorts", "widenings", "zero_distance", "bad_mass")
_SN_FIRST_CAP = 1 << 16


def _sn_call(points, masses, stars, ptypes, velocities, mass_displaced, supernova_energy):
    """sphx_supernova_impulse on host arrays -> (velocities or None, sel_count, sel_ids, d_vels, true_mass, vel, counts)."""
    import re
    pts = f64(points)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError("points must be (N, 3)")
    n = pts.shape[0]
    m, pt = f64(masses, (n,)), f64(ptypes, (n,))
    ku = i64(stars)
    if ku.ndim != 1:
        raise ValueError("supernova_pos must be a scalar or a 1-D array of indices")
    n_sn = ku.shape[0]
    v = None if velocities is None else np.array(f64(velocities, (n, 3)))        # (a copy: the call adds in place)
    g = globals()
    M = float(g["mass_displaced"] if mass_displaced is None else mass_displaced)
    E = float(g["supernova_energy"] if supernova_energy is None else supernova_energy) * SN_KICK_FRACTION
    most = int(np.count_nonzero(pt == 0)) * n_sn
    cap = min(most, _SN_FIRST_CAP)
    c_ = context()
    while True:
        sel_count = np.zeros(n_sn, dtype=np.int64)
        sel_ids = np.zeros(max(cap, 1), dtype=np.int64); d_vels = np.zeros((max(cap, 1), 3))
        true_mass = np.zeros(n_sn); vel = np.zeros(n_sn)
        counts = np.zeros(len(SN_COUNTS), dtype=np.int64)
        rc = c_.lib.sphx_supernova_impulse(c_.h, n, dp(pts), dp(m), dp(pt), n_sn, ip(ku), M, E, dp(v), cap, ip(sel_count), ip(sel_ids),
                                           dp(d_vels), dp(true_mass), dp(vel), ip(counts))
        if rc == -1 and cap < most:
            # (cap too small: the error text names the size needed, include/sphx.h)
            need = re.search(r"the selections hold (\d+) rows", (c_.lib.sphx_last_error(c_.h) or b"").decode())
            if need:
                cap = int(need.group(1))
                continue
        c_.check(rc)
        break
    total = int(sel_count.sum())
    return v, sel_count, sel_ids[:total], d_vels[:total], true_mass, vel, dict(zip(SN_COUNTS, (int(x) for x in counts)))


def supernova_impulse(points, masses, supernova_pos, ptypes, mass_displaced=None, supernova_energy=None, full=False):
    """nsc:1192-1204 for one star (a scalar supernova_pos) -> (d_vels (n_sel,3), selected_points (n_sel,) int64): the
    nearest gas rows whose running mass stays below mass_displaced (nsc:1193) and their radial kick.  Rows at bit-equal
    distance are taken in ascending index (the reference's argsort leaves their order open); include/sphx.h,
    sphx_supernova_impulse, lists the rest.  mass_displaced and supernova_energy default to the module's values, read at
    call time.  full=True appends a dict: true_mass, vel, counts (SN_COUNTS)."""
    if np.ndim(supernova_pos) != 0:
        raise ValueError("supernova_pos must be a scalar (supernova_impulses takes an array of stars)")
    _, _, ids, d_vels, tm, vel, counts = _sn_call(points, masses, [int(supernova_pos)], ptypes, None, mass_displaced, supernova_energy)
    if full:
        return d_vels, ids, {"true_mass": float(tm[0]), "vel": float(vel[0]), "counts": counts}
    return d_vels, ids


def supernova_impulses(points, masses, supernova_pos, ptypes, velocities, mass_displaced=None, supernova_energy=None, full=False):
    """The driver's loop drv:350-352 over the stars supernova_pos, in their order -> (velocities_new (N,3), selections):
    selections[t] = (d_vels, selected_points) of star t as supernova_impulse returns them; a star's kicks are added on top
    of the previous stars'.  The given velocities are not modified.  full=True appends a dict: true_mass, vel (per star),
    counts (SN_COUNTS)."""
    v, sel_count, ids, d_vels, tm, vel, counts = _sn_call(points, masses, np.atleast_1d(supernova_pos), ptypes, velocities,
                                                          mass_displaced, supernova_energy)
    ends = np.cumsum(sel_count)
    sels = [(d_vels[e - c:e], ids[e - c:e]) for c, e in zip(sel_count, ends)]
    if full:
        return v, sels, {"true_mass": tm, "vel": vel, "counts": counts}
    return v, sels


def sn_last_timing():
    """Device time of the last supernova_impulse(s) call of this module, from HIP events and added up over its stars
    (include/sphx.h sphx_sn_last_timing) -> dict of ms: keys, bound, compact, sort, walk, kick."""
    return _last_timing("sphx_sn_last_timing", ("keys", "bound", "compact", "sort", "walk", "kick"))


# ==============================================================================================
# Thermal / chemical sputtering and reuptake: chemisputtering_2 (nsc:1265-1416)
# ==============================================================================================
CHEM_COUNTS = ("rows", "pairs", "clamp1", "clamp2", "clamp3", "columns_corrected", "rounds")


def chem_table(S, given, name):
    """A per-species table of length S as float64: `given`, or the module's `name` (the reference's 15 entries, cut to S
    where S < 15; S > 15 needs a given one)."""
    t = f64(globals()[name] if given is None else given)
    if given is None and S < t.shape[0]:
        t = np.ascontiguousarray(t[:S])
    if t.shape != (S,):
        raise ValueError("%s must hold S = %d entries" % (name, S))
    return t


def chemisputtering_2(points, neighbor, mass, f_un, mu_array, sizes, T, particle_type, d=None, dt=None, mu_specie=None,
                      mineral_densities=None, sputtering_yields=None, mrn_constants=None, full=False):
    """nsc:1265-1416 -> (mass_new (N,), f_un_new (N,S)); full=True appends a dict of the counts (CHEM_COUNTS).  d and dt
    default to the module attributes, read at call time as the reference reads its globals (the driver assigns both);
    the tables default to the module's, which are the reference's.  The reference's prints are dropped.  The rows'
    order dependence is resolved by rounds on the device that end on the sequential result; include/sphx.h,
    sphx_chemisputtering_2, has the formulas and lists the quirks kept."""
    nb, n, K = _nk(neighbor)
    pts, m, mu = f64(points, (n, 3)), f64(mass, (n,)), f64(mu_array, (n,))
    h, temp, pt = f64(sizes, (n,)), f64(T, (n,)), f64(particle_type, (n,))
    fun = f64(f_un)
    if fun.ndim != 2 or fun.shape[0] != n:
        raise ValueError("f_un must be (N, S)")
    S = fun.shape[1]
    g = globals()
    mus = chem_table(S, mu_specie, "mu_specie")
    dens = chem_table(S, mineral_densities, "mineral_densities")
    ys = chem_table(S, sputtering_yields, "sputtering_yields")
    mrn = f64(g["mrn_constants"] if mrn_constants is None else mrn_constants, (2,))
    tstep = float(g["dt"] if dt is None else dt)
    mass_new = np.empty(n); f_new = np.empty((n, S))
    counts = np.zeros(len(CHEM_COUNTS), dtype=np.int64) if full else None
    c_ = context()
    c_.check(c_.lib.sphx_chemisputtering_2(c_.h, n, K, S, dp(pts), ip(nb), dp(m), dp(fun), dp(mu), dp(h), dp(temp), dp(pt), _d(d),
                                           tstep, dp(mus), dp(dens), dp(ys), dp(mrn), float(k), float(amu), float(m_0),
                                           dp(mass_new), dp(f_new), ip(counts)))
    if full:
        return mass_new, f_new, dict(zip(CHEM_COUNTS, (int(v) for v in counts)))
    return mass_new, f_new


def chem_last_timing():
    """Device time of the last chemisputtering_2 call of this module, from HIP events (include/sphx.h
    sphx_chem_last_timing) -> dict of ms: upload, rows, reverse, rounds, closing."""
    return _last_timing("sphx_chem_last_timing", ("upload", "rows", "reverse", "rounds", "closing"))


# ==============================================================================================
# The dust phase of the time loop: code_running.py:399-435
# ==============================================================================================
PHASE_TOTALS = ("mass_before", "mass_after_chem", "mass_after", "mass_reduction", "mass_increase", "mass_change")
PHASE_COUNTS = ("masses_reset", "nan_filled")


def dust_bookkeeping(mass, mu_array, f_un, frac_destruction, frac_reuptake, mass_before=None, mu_specie=None, gamma=None,
                     crit_mass=None):
    """drv:412-433 -> (mass, f_un, mu_array, gamma_array, totals).  mass and f_un are chemisputtering_2's outputs,
    mu_array the one that went into the phase, the fractions supernova_destruction's.  totals: dict of the numbers the
    driver prints (PHASE_TOTALS, in kg; mass_before is NaN unless the masses from before chemisputtering are given) and
    the counts PHASE_COUNTS.  The tables and crit_mass default to the module's, read at call time.  include/sphx.h,
    sphx_dust_bookkeeping, has the formulas and the quirks kept."""
    fun = f64(f_un)
    if fun.ndim != 2:
        raise ValueError("f_un must be (N, S)")
    n, S = fun.shape
    m, mu = f64(mass, (n,)), f64(mu_array, (n,))
    destr, reup = f64(frac_destruction, (n, S)), f64(frac_reuptake, (n, S))
    mb = None if mass_before is None else f64(mass_before, (n,))
    g = globals()
    mus = chem_table(S, mu_specie, "mu_specie")
    gam = chem_table(S, gamma, "gamma")
    cm = float(g["crit_mass"] if crit_mass is None else crit_mass)
    m_out = np.empty(n); f_out = np.empty((n, S)); mu_out = np.empty(n); g_out = np.empty(n)
    tot = np.zeros(len(PHASE_TOTALS)); cnt = np.zeros(len(PHASE_COUNTS), dtype=np.int64)
    c_ = context()
    c_.check(c_.lib.sphx_dust_bookkeeping(c_.h, n, S, dp(m), dp(mu), dp(fun), dp(destr), dp(reup), dp(mb), dp(mus), dp(gam), cm,
                                          dp(m_out), dp(f_out), dp(mu_out), dp(g_out), dp(tot), ip(cnt)))
    totals = dict(zip(PHASE_TOTALS, (float(v) for v in tot)))
    totals.update(zip(PHASE_COUNTS, (int(v) for v in cnt)))
    return m_out, f_out, mu_out, g_out, totals


def normalise_rows(f_un):
    """drv:399 / drv:424: every row divided by its sum, the sum taken over the species one by one (the order the
    resident call's kernel adds them in; np.sum pairs them differently from eight species on)."""
    fun = f64(f_un)
    tot = fun[:, 0].copy()
    for t in range(1, fun.shape[1]):
        tot = tot + fun[:, t]
    return fun / tot[:, None]


def dust_phase(points, velocities, neighbor, mass, f_un, mu_array, sizes, T, particle_type, d=None, dt=None, mu_specie=None,
               gamma=None, mineral_densities=None, sputtering_yields=None, mrn_constants=None, crit_mass=None,
               critical_density=None, species_curve=None, guard="count", full=False):
    """The block code_running.py:399-435 as a chain of the array calls - density, chemisputtering_2,
    supernova_destruction, dust_bookkeeping - on the caller's arrays and `neighbor` -> (mass, f_un, mu_array, gamma_array,
    totals); full=True appends a dict of the stage outputs (density, mass_chem, f_un_chem, frac_destruction,
    frac_reuptake, chem_counts, dust_counts).  dust_density and num_dens (drv:401-402) are dead in the block and are not
    formed; cross_array and optical_depth (drv:434-435) are left to the caller.  Simulation.dust_phase is the same on the
    resident state, bit for bit."""
    m0 = f64(mass)
    fun = normalise_rows(f_un)                                                         # drv:399
    dens = density(points, m0, particle_type, neighbor, d=d)                           # drv:400
    m1, f1, cc = chemisputtering_2(points, neighbor, m0, fun, mu_array, sizes, T, particle_type, d=d, dt=dt, mu_specie=mu_specie,
                                   mineral_densities=mineral_densities, sputtering_yields=sputtering_yields,
                                   mrn_constants=mrn_constants, full=True)             # drv:407-408
    destr, reup, dc = supernova_destruction(points, velocities, neighbor, m1, f1, mu_array, sizes, dens, particle_type,
                                            crit_mass=crit_mass, critical_density=critical_density, species_curve=species_curve,
                                            guard=guard, full=True)                    # drv:411
    out = dust_bookkeeping(m1, mu_array, f1, destr, reup, mass_before=m0, mu_specie=mu_specie, gamma=gamma, crit_mass=crit_mass)
    if full:
        return out + (dict(density=dens, mass_chem=m1, f_un_chem=f1, frac_destruction=destr, frac_reuptake=reup,
                           chem_counts=cc, dust_counts=dc),)
    return out


def phase_tables(S, dt=None, mu_specie=None, gamma=None, mineral_densities=None, sputtering_yields=None, mrn_constants=None,
                 crit_mass=None, critical_density=None, species_curve=None, guard="count"):
    """The table and scalar arguments of sphx_state_dust_phase from the module's values, read at call time (what
    dust_phase's stages read one by one) -> dict."""
    if not isinstance(guard, str) or guard not in DUST_GUARDS:
        raise ValueError("guard must be 'count' or 'fraction', not %r" % (guard,))
    g = globals()
    return dict(dt=float(g["dt"] if dt is None else dt), mu_specie=chem_table(S, mu_specie, "mu_specie"),
                gamma=chem_table(S, gamma, "gamma"), mineral_densities=chem_table(S, mineral_densities, "mineral_densities"),
                sputtering_yields=chem_table(S, sputtering_yields, "sputtering_yields"),
                mrn=f64(g["mrn_constants"] if mrn_constants is None else mrn_constants, (2,)),
                crit_mass=float(g["crit_mass"] if crit_mass is None else crit_mass),
                critical_density=float(g["critical_density"] if critical_density is None else critical_density),
                species_curve=dust_species_curve(S, species_curve), guard=DUST_GUARDS[guard],
                knots=tuple(np.array(a, dtype=np.float64) for a in (DUST_KNOTS_V, DUST_KNOTS_C, DUST_KNOTS_SI)))


# ==============================================================================================
# The radiative block of the time loop: code_running.py:247-316
# ==============================================================================================
planck_h = 6.62607015e-34                       # nsc:26 (scipy.constants.h)
sb = 5.6703744191844314e-08                     # nsc:23
wien = 0.0028977719551851727                    # nsc:28
t_cmb = 2.732                                   # nsc:33
t_solar = 5776                                  # nsc:34
supernova_energy = 1e44                         # nsc:35
cross_sections = np.array([6.3e-22, 6.3e-22, 6.3e-22, 1e-60, 1e-60, 1.e-60, 6.65e-60 * 80] + [0.] * 8) / 80. + 1e-80       # nsc:42
destruction_energies = np.array([7.2418e-19, 3.93938891e-18, 2.18e-18, 10000, 10000, 8.71584082e-18] + [10000] * 9)      # nsc:43
RADPHASE_TOTALS = ("E_before", "E_after_heating", "E_after_cooling")
RADPHASE_COUNTS = ("E_raised", "E_lowered", "T_raised", "T_lowered")


def driver_cross_sections(S=15):
    """The per-species cross-sections of the DRIVER (drv:46, 58): the module's plus sigma_effective.  The bookkeeping of
    drv:260 / 285 forms cross_array with these; rad_heating's own chemistry (nsc:979) reads the module's.  The effective
    cross-section is formed factor by factor as nsc:73 has it (this module's sigma_effective multiplies by the ratio of
    the two differences, an ulp away on some species), so that the table has the driver's bits."""
    lo, hi = _mrn_limits(mrn_constants)
    seff = chem_table(S, None, "mu_specie") * amu / chem_table(S, None, "mineral_densities") * (3. / 4.) * \
        -(hi ** -0.5 - lo ** -0.5) / (hi ** 0.5 - lo ** 0.5)
    return chem_table(S, None, "cross_sections") + seff


def _mass_laws(base_imf):
    """Coefficient and exponent of the mass-luminosity and mass-radius power laws (nsc:175-188, 210-223), per star: the
    luminosity law breaks at 0.7, the radius law at 1.66 solar masses; a NaN mass falls on neither side and gets zeros."""
    b = f64(base_imf).reshape(-1)
    laws = []
    for brk, lo, hi in ((0.7, (0.35, 2.62), (1.02, 3.92)), (1.66, (1.06, 0.945), (1.2916594319, 0.555))):
        coeff, expo = np.zeros(b.shape[0]), np.zeros(b.shape[0])
        coeff[b < brk], expo[b < brk] = lo
        coeff[b >= brk], expo[b >= brk] = hi
        laws += [coeff, expo]
    return (b,) + tuple(laws)


def luminosity_relation(base_imf, lifetime=0):
    """nsc:174-200 without its unused `imf` argument -> luminosity in solar units of stars of base_imf solar masses, or
    with lifetime=1 their lifetime in units of 1e10 years, floored at 3.6e-4."""
    b, cl, el, _, _ = _mass_laws(base_imf)
    if lifetime == 0:
        return cl * b ** el
    if lifetime == 1:
        life = cl ** (-1) * b ** (1 - el)
        life[life < 3.6e-4] = 3.6e-4
        return life
    return None


def rad_setup(ptypes, masses, supernova_pos, dt, rng=np.random):
    """nsc:897-921, the random half of rad_heating -> (source_ids, luminosities, target_ids): caller indices of the
    selected stars, their luminosities (solar units, renormalised to the total of ALL stars), caller indices of the
    sampled non-star particles.  rng.rand(n_stars) is drawn first and rng.rand(n_nonstar) second, as the reference
    draws them: with the global np.random seeded alike, the selection is the reference's.  Quirks kept: a star is
    taken with probability m / (4 solar masses) + n_stars^-0.5; none drawn -> all stars; a star listed in supernova_pos
    adds 0.264 supernova_energy / solar_luminosity / dt; a non-star particle is sampled with probability
    n_nonstar^-0.65, all of them only when there is no star at all."""
    pt, m = f64(ptypes).reshape(-1), f64(masses).reshape(-1)
    stars, others = np.nonzero(pt == 1)[0], np.nonzero(pt != 1)[0]
    n_s, n_o = len(stars), len(others)
    msun = m[stars] / solar_mass
    chosen = np.arange(n_s)
    if n_s > 0:
        chosen = np.nonzero(rng.rand(n_s) < (m[stars] / (4 * solar_mass)) + n_s ** -0.5)[0]
        if len(chosen) == 0:
            chosen = np.arange(n_s)
    exploding = np.zeros(len(m))
    exploding[np.asarray(supernova_pos, dtype=np.int64)] += 1
    base = luminosity_relation(msun[chosen]) + 0.264 * supernova_energy / solar_luminosity / dt * exploding[stars][chosen]
    total = np.sum(luminosity_relation(msun))
    with np.errstate(all="ignore"):
        lum = base / np.sum(base) * total
    targets = others[:0]
    if n_o > 0:
        targets = others[rng.rand(n_o) < n_o ** -0.65]
        if len(chosen) == 0:
            targets = others
    return stars[chosen].astype(np.int64), lum, targets.astype(np.int64)


def planck_law(temp, wl, dwl):
    """nsc:202-207: the black-body spectrum at `temp` on the wavelengths wl, its first entry zeroed, normalised over dwl."""
    with np.errstate(all="ignore"):
        emission = np.nan_to_num((2 * planck_h * c ** 2 / wl ** 5) / (np.exp(planck_h * c / (wl * k * temp)) - 1))
        emission[0] = 0
        return np.nan_to_num(emission / np.sum(emission * dwl))


def overall_spectrum(base_imf):
    """nsc:209-245 with imf = 1 per star (all rad_heating asks for) -> (wl, spectrum, dwl): the stars' black bodies at
    the temperatures of the two power laws, weighted by luminosity, on 10000 wavelengths spaced by logarithm around the
    solar Wien peak."""
    b, cl, el, cr, er = _mass_laws(base_imf)
    lum = cl * b ** el
    temp = (cl / cr) ** (1. / 4.) * b ** ((el - er) / 4.)
    peak = np.log10(wien / t_solar)
    wl = np.logspace(peak - 5, peak + 3, 10000)
    dwl = np.append(wl[0], np.diff(wl))
    spec = np.zeros(len(wl))
    for u in range(len(b)):
        spec += np.nan_to_num(np.nan_to_num(planck_law(temp[u] * t_solar, wl, dwl)) * 1. * lum[u])
    with np.errstate(all="ignore"):
        spec /= np.sum(dwl * spec)
        spec *= np.sum(lum) / np.sum(b) * solar_luminosity / solar_mass
    return wl, spec, dwl


def stellar_spectrum(star_masses, destruction_energies=None):
    """nsc:967-976 -> (frac_dest (S,), photons_per_joule).  star_masses: masses[ptypes == 1], in kg.  frac_dest[t] is
    the share of the stars' summed spectrum (weighted by wavelength and bin width) short of species t's destruction
    wavelength; photons_per_joule the scalar nsc:976 multiplies lf2 by to get n_photons."""
    de = f64(globals()["destruction_energies"] if destruction_energies is None else destruction_energies)
    wl, spec, dwl = overall_spectrum(f64(star_masses) / solar_mass)
    hc = planck_h * c
    limit = de ** (-1) * hc
    weighted = spec * dwl * wl
    with np.errstate(all="ignore"):
        frac = np.array([np.sum(weighted[wl < limit[t]]) for t in range(len(limit))])
        frac /= np.sum(weighted)
        ppj = np.sum(wl * spec * dwl / hc) / np.sum(spec * dwl)
    return frac, float(ppj)


def _radphase_tables(S, mu_specie=None, gamma=None, cross_sections=None):
    cs = driver_cross_sections(S) if cross_sections is None else chem_table(S, cross_sections, "cross_sections")
    return chem_table(S, mu_specie, "mu_specie"), chem_table(S, gamma, "gamma"), cs


def _n_gas(pt, what, arr, width=None):
    g = int(np.count_nonzero(pt != 1))
    a = f64(arr)
    if a.shape != ((g,) if width is None else (g, width)):
        raise ValueError("%s must hold one row per particle with ptypes != 1 (%d)" % (what, g))
    return g, a


def rad_ionise(f_un, ptypes, masses, lf2, frac_dest, photons_per_joule, mu_specie=None, cross_sections=None, full=False):
    """nsc:976-1012, the photoionisation chemistry of rad_heating -> f_un_new (N,S): the second element of rad_heating's
    return tuple.  lf2 is rad_transfer's (over the particles with ptypes != 1), frac_dest and photons_per_joule
    stellar_spectrum's.  cross_sections defaults to the MODULE's (nsc:42), as inside the reference.  full=True appends
    frac_destroyed_by_species[:, :3] (G,3), the three columns the reactions read.  include/sphx.h, sphx_rad_ionise."""
    fun = f64(f_un)
    if fun.ndim != 2:
        raise ValueError("f_un must be (N, S)")
    n, S = fun.shape
    pt, m = f64(ptypes, (n,)), f64(masses, (n,))
    g, lf = _n_gas(pt, "lf2", lf2)
    fd = f64(frac_dest, (S,))
    mus, cs = chem_table(S, mu_specie, "mu_specie"), chem_table(S, cross_sections, "cross_sections")
    out = np.empty((n, S)); frac = np.empty((g, 3)) if full else None
    c_ = context()
    c_.check(c_.lib.sphx_rad_ionise(c_.h, n, S, g, dp(fun), dp(pt), dp(m), dp(lf), dp(fd), float(photons_per_joule), dp(mus), dp(cs),
                                    float(amu), dp(out), dp(frac)))
    return (out, frac) if full else out


def _radphase_totals(tot, cnt, names):
    out = dict(zip(names, (float(v) for v in tot)))
    out.update(zip(RADPHASE_COUNTS, (int(v) for v in cnt)))
    return out


def rad_heat_bookkeeping(f_un, ptypes, masses, mu_before, E_internal, T, lf2, t_max, t_cmb=None, mu_specie=None, gamma=None,
                         cross_sections=None):
    """drv:258-273 -> (mu_array, gamma_array, cross_array, E_internal, T, totals).  f_un is rad_ionise's, mu_before the
    mu_array from before the heating (N_PART at drv:268 is drv:248's), lf2 rad_transfer's.  t_max is undefined in the
    driver and has no default here.  cross_sections defaults to the DRIVER's (driver_cross_sections).  totals: the sum of
    E_internal before and after, and how many entries each clamp moved (RADPHASE_COUNTS).  include/sphx.h,
    sphx_rad_heat_bookkeeping."""
    fun = f64(f_un)
    if fun.ndim != 2:
        raise ValueError("f_un must be (N, S)")
    n, S = fun.shape
    pt, m, mub = f64(ptypes, (n,)), f64(masses, (n,)), f64(mu_before, (n,))
    E, temp = f64(E_internal, (n,)), f64(T, (n,))
    g, lf = _n_gas(pt, "lf2", lf2)
    mus, gam, cs = _radphase_tables(S, mu_specie, gamma, cross_sections)
    outs = [np.empty(n) for _ in range(5)]
    tot = np.zeros(2); cnt = np.zeros(4, dtype=np.int64)
    c_ = context()
    c_.check(c_.lib.sphx_rad_heat_bookkeeping(c_.h, n, S, g, dp(fun), dp(pt), dp(m), dp(mub), dp(E), dp(temp), dp(lf), dp(mus), dp(gam),
                                              dp(cs), float(globals()["t_cmb"] if t_cmb is None else t_cmb), float(t_max), float(k),
                                              float(m_h), *([dp(a) for a in outs] + [dp(tot), ip(cnt)])))
    return tuple(outs) + (_radphase_totals(tot, cnt, ("E_before", "E_after")),)


def rad_cool_bookkeeping(final_comp, energy, ptypes, masses, sizes, E_internal, T, velocities, lf2, momentum, dt, t_max,
                         cooling_timescale, t_cmb=None, mu_specie=None, gamma=None, cross_sections=None):
    """drv:283-311 -> (mu_array, gamma_array, cross_array, E_internal, T, velocities, totals).  final_comp and energy are
    rad_cooling's first two results, lf2 and momentum rad_transfer's, E_internal and T rad_heat_bookkeeping's.  t_max and
    cooling_timescale are undefined in the driver and have no default here.  include/sphx.h, sphx_rad_cool_bookkeeping."""
    fun = f64(final_comp)
    if fun.ndim != 2:
        raise ValueError("final_comp must be (N, S)")
    n, S = fun.shape
    pt, m, h, en = f64(ptypes, (n,)), f64(masses, (n,)), f64(sizes, (n,)), f64(energy, (n,))
    E, temp, vel = f64(E_internal, (n,)), f64(T, (n,)), f64(velocities, (n, 3))
    g, lf = _n_gas(pt, "lf2", lf2)
    _, mom = _n_gas(pt, "momentum", momentum, 3)
    mus, gam, cs = _radphase_tables(S, mu_specie, gamma, cross_sections)
    outs = [np.empty(n) for _ in range(5)] + [np.empty((n, 3))]
    tot = np.zeros(2); cnt = np.zeros(4, dtype=np.int64)
    c_ = context()
    c_.check(c_.lib.sphx_rad_cool_bookkeeping(c_.h, n, S, g, dp(fun), dp(en), dp(pt), dp(m), dp(h), dp(E), dp(temp), dp(vel), dp(lf),
                                              dp(mom), dp(mus), dp(gam), dp(cs), float(dt),
                                              float(globals()["t_cmb"] if t_cmb is None else t_cmb), float(t_max),
                                              float(cooling_timescale), float(sb), float(k), float(m_h),
                                              *([dp(a) for a in outs] + [dp(tot), ip(cnt)])))
    return tuple(outs) + (_radphase_totals(tot, cnt, ("E_before", "E_after")),)


def row_ratio(f_un, table):
    """sum_t f_un[i,t] table[t] / sum_t f_un[i,t] per particle, both sums taken over the species one by one (the order the
    library's kernels add a row in; np.sum pairs them differently from eight species on)."""
    fun = f64(f_un)
    cols = np.ascontiguousarray(fun.T)               # (contiguous columns: the sums below run over whole arrays)
    num, den = cols[0] * table[0], cols[0].copy()
    for t in range(1, cols.shape[0]):
        num = num + cols[t] * table[t]
        den = den + cols[t]
    with np.errstate(all="ignore"):
        return num / den


def cross_array_of(f_un, cross_sections=None):
    """cross_array as drv:434 leaves it for rad_heating: row_ratio of f_un with the driver's cross-sections."""
    S = f64(f_un).shape[1]
    return row_ratio(f_un, driver_cross_sections(S) if cross_sections is None else chem_table(S, cross_sections, "cross_sections"))


def rad_phase(points, velocities, neighbor, mass, f_un, mu_array, sizes, T, E_internal, particle_type, source_ids, luminosities,
              target_ids, frac_dest, photons_per_joule, dt, d, t_max, cooling_timescale, mode="line", full=False, t_cmb=None,
              mu_specie=None, gamma=None, cross_sections=None, driver_cross=None):
    """The block code_running.py:247-316 with N_RADIATIVE = 1 as a chain of the array calls - rad_transfer, rad_ionise,
    rad_heat_bookkeeping, rad_cooling, rad_cool_bookkeeping - on the caller's arrays and `neighbor`
    -> (f_un, mu_array, gamma_array, E_internal, T, velocities, totals); full=True appends a dict of the stage outputs.
    source_ids, luminosities, target_ids are rad_setup's, frac_dest and photons_per_joule stellar_spectrum's.
    cross_sections is the module's table (rad_ionise), driver_cross the driver's (the bookkeeping and the cross_array
    that goes into rad_transfer).  With no star (drv:243) the driver skips the block: no GPU call is made, f_un, mu_array,
    E_internal, T and velocities come back as given, gamma_array - which is no input - is row_ratio(f_un, gamma), what
    drv:162 formed it as from the same f_un, and totals is {"skipped": True}."""
    pt = f64(particle_type)
    pts = f64(points)
    if not np.any(pt == 1):
        gam0 = row_ratio(f_un, chem_table(f64(f_un).shape[1], gamma, "gamma"))
        return (f64(f_un), f64(mu_array), gam0, f64(E_internal), f64(T), f64(velocities), dict(skipped=True)) + ((dict(),) if full else ())
    src = np.asarray(source_ids, dtype=np.int64); dst = np.asarray(target_ids, dtype=np.int64)
    cross0 = cross_array_of(f_un, driver_cross)
    lf2, mom, ext = rad_transfer(pts, pt, mass, sizes, cross0, mu_array, pts[src], luminosities, pts[dst], dt, mode=mode)
    f1, frac = rad_ionise(f_un, pt, mass, lf2, frac_dest, photons_per_joule, mu_specie=mu_specie, cross_sections=cross_sections,
                          full=True)
    mu1, g1, cr1, E1, T1, tot1 = rad_heat_bookkeeping(f1, pt, mass, mu_array, E_internal, T, lf2, t_max, t_cmb=t_cmb,
                                                      mu_specie=mu_specie, gamma=gamma, cross_sections=driver_cross)
    final, energy, rec = rad_cooling(pts, pt, mass, sizes, cr1, f1, neighbor, mu1, T1, dt, d=d)
    mu2, g2, cr2, E2, T2, v2, tot2 = rad_cool_bookkeeping(final, energy, pt, mass, sizes, E1, T1, velocities, lf2, mom, dt, t_max,
                                                          cooling_timescale, t_cmb=t_cmb, mu_specie=mu_specie, gamma=gamma,
                                                          cross_sections=driver_cross)
    totals = dict(skipped=False, E_before=tot1["E_before"], E_after_heating=tot1["E_after"], E_after_cooling=tot2["E_after"])
    for nm in RADPHASE_COUNTS:
        totals["heat_" + nm], totals["cool_" + nm] = tot1[nm], tot2[nm]
    out = (final, mu2, g2, E2, T2, v2, totals)
    if full:
        out += (dict(cross_array=cross0, lf2=lf2, momentum=mom, extinction=ext, f_un_ionised=f1, frac_destroyed=frac, mu_heat=mu1,
                     gamma_heat=g1, cross_heat=cr1, E_heat=E1, T_heat=T1, final_comp=final, energy=energy, rec_array=rec,
                     cross_array_out=cr2),)
    return out


def radphase_last_timing():
    """Device time of the last rad_ionise / rad_heat_bookkeeping / rad_cool_bookkeeping call of this module, from HIP
    events (include/sphx.h sphx_radphase_last_timing) -> dict of ms: upload, kernel, sums, download."""
    return _last_timing("sphx_radphase_last_timing", ("upload", "kernel", "sums", "download"))


# ==============================================================================================
# The explosion itself and the insertion of its particles: supernova_explosion (nsc:820-882), drv:361-396
# ==============================================================================================
# Host code, on the few rows of the exploding stars: the one part of this module that computes in NumPy.  It restates the
# reference's statements with the same NumPy operations on arrays of the same layout, so the bits are the reference's.
SN_PROGEN_MASS = (0, 20, 25, 30, 35, 40)                                        # nsc:82, solar masses
# nsc:81-99, the mixed CCSN dust yields by species: None is the reference's zero_function, an entry the yields at
# SN_PROGEN_MASS (written as the reference writes them: 7*10**(-2) is not the double 0.07)
SN_YIELDS = (None, None, None, None, None, None,
             (6 * 10 ** (-2), 10 ** (-1) * 1.5, 2 * 10 ** (-1), 8 * 10 ** (-1), 1, 1),                     # Mg2SiO4
             (4 * 10 ** (-2), 4 * 10 ** (-1), 4.1 * 10 ** (-1), 5 * 10 ** (-1), 10 ** (-1) * 8, 10 ** (-1) * 8),   # SiO2
             None, None,
             (10 ** (-2), 7 * 10 ** (-2), 7 * 10 ** (-2), 7 * 10 ** (-2), 7 * 10 ** (-2), 7 * 10 ** (-2)),  # Fe
             (2 * 10 ** (-2), 5 * 10 ** (-2), 6 * 10 ** (-2), 9 * 10 ** (-3), 0, 0),                        # MgSiO3
             None, None)
SN_REMNANT_MASS = 2.                                                            # nsc:837, 849: solar masses left as the star
SN_DUST_ROW_MASS = 0.05                                                         # nsc:840: solar masses per dust row
EXPLOSION_FIELDS = ("dust_comps", "gas_comps", "star_comps", "dust_mass", "gas_mass", "stars_mass", "newpoints", "newvels",
                    "newgastype", "newdusttype", "new_eint_stars", "new_eint_dust", "new_eint_gas", "supernova_pos", "dustpoints",
                    "dustvels")


def sn_yield_table(S, yields=None):
    """The per-species yields as a list of S entries, each None ("none") or the six values at SN_PROGEN_MASS: `yields`, or
    the reference's 14-entry tuple padded with None to S (as dust_species_curve pads)."""
    y = list(SN_YIELDS if yields is None else yields)
    if yields is None:
        y = y[:S] + [None] * (S - len(y))
    if len(y) != S:
        raise ValueError("yields must hold S = %d entries" % S)
    out = []
    for e in y:
        if e is None:
            out.append(None)
            continue
        e = np.array(e, dtype=np.float64)
        if e.shape != (len(SN_PROGEN_MASS),):
            raise ValueError("a yield entry holds %d values at SN_PROGEN_MASS" % len(SN_PROGEN_MASS))
        out.append(e)
    return out


def _interp_linear(x, y, x_new):
    """scipy.interpolate.interp1d(x, y, kind='linear')(x_new) with its default bounds_error: the same statements
    (searchsorted, clip, slope = (y_hi - y_lo) / (x_hi - x_lo), slope (x_new - x_lo) + y_lo), so the same bits."""
    if np.any(x_new < x[0]) or np.any(x_new > x[-1]):
        raise ValueError("A value in x_new is outside the interpolation range [%g, %g] solar masses." % (x[0], x[-1]))
    idx = np.searchsorted(x, x_new).clip(1, len(x) - 1).astype(int)
    lo, hi = idx - 1, idx
    x_lo, x_hi, y_lo, y_hi = x[lo], x[hi], y[lo], y[hi]
    slope = (y_hi - y_lo) / (x_hi - x_lo)
    return slope * (x_new - x_lo) + y_lo


def supernova_explosion(mass, points, velocities, E_internal, supernova_pos, f_un, d_0=None, noise_dust=None, noise_gas=None,
                        yields=None, full=False):
    """nsc:820-882 -> the reference's 16-entry tuple (EXPLOSION_FIELDS) for the stars supernova_pos.  Kept as committed:
    grsum, drsum and trsum run over ALL stars; dust_mass is uniform over all dust rows; a star sheds
    int(dust_masses / (0.05 solar_mass)) dust rows and one gas row; stars_mass = 2 solar masses; new_eint_gas = E / 2;
    star_comps is gas_comps.  d_0 defaults to the module's (drv:70).  The noise is drawn as the reference draws it,
    np.random.normal(size=(n_dust, 3)) and then (n_sn, 3): under its seed the positions are its bits; noise_dust and
    noise_gas (standard normal, of those shapes) replace the draws.  yields: sn_yield_table.  A progenitor outside
    [0, 40] solar masses raises ValueError, as the reference's interp1d does.
    Two readings are this module's: every dust row takes its OWN star's velocity (nsc:858-859 indexes with
    the stale `position`: with two or more stars every dust row gets the last star's velocity, and their number is
    wrong); and an event without a single dust row, where the reference raises in np.vstack, gives empty dust arrays.
    The inputs are not modified.  full=True appends a dict: dust_len (the dust rows per star)."""
    m, E = f64(mass), f64(E_internal)
    pts, vel = f64(points), f64(velocities)
    fun = f64(f_un)
    sp = np.ascontiguousarray(np.asarray(supernova_pos, dtype=np.int64).reshape(-1))
    n_sn, S = sp.shape[0], fun.shape[1]
    d0 = globals()["d_0"] if d_0 is None else d_0
    if d0 is None:
        raise NameError("name 'd_0' is not defined (assign nsc.d_0 as sph/code_running.py:70 does)")
    d0 = float(d0)
    table = sn_yield_table(S, yields)
    knots = np.array(SN_PROGEN_MASS)
    gas_release = fun[sp]                                                        # nsc:823 (a copy)
    grsum = np.sum(gas_release)
    rel = m[sp] / solar_mass
    dust_release = np.array([np.zeros(len(rel)) if y is None else _interp_linear(knots, y, rel) for y in table]).T     # nsc:826
    drsum = np.sum(dust_release)
    total_release = dust_release + gas_release
    trsum = np.sum(total_release)
    gas_release /= grsum
    dust_release /= drsum
    dust_masses = (m[sp] - SN_REMNANT_MASS * solar_mass) * drsum / trsum
    gas_masses = (m[sp] - SN_REMNANT_MASS * solar_mass) * grsum / trsum
    dust_len = np.array(dust_masses / (SN_DUST_ROW_MASS * solar_mass)).astype('int')
    n_dust = int(np.sum(dust_len))
    stars_mass = np.ones(n_sn) * 2 * solar_mass
    if n_dust > 0:
        dust_mass = np.ones(n_dust) * np.sum(dust_masses) / n_dust
        noise = np.random.normal(size=(n_dust, 3)) if noise_dust is None else f64(noise_dust, (n_dust, 3))
        dustpoints = np.vstack([pts[sp[t]] for t in range(n_sn) for _ in range(dust_len[t])]) + noise * d0
        dustvels = np.vstack([vel[sp[t]] for t in range(n_sn) for _ in range(dust_len[t])])
        dust_comps = np.array([dust_release[t] for t in range(n_sn) for _ in range(dust_len[t])])
    else:
        dust_mass = np.zeros(0)
        dustpoints, dustvels, dust_comps = np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, S))
    noise = np.random.normal(size=(n_sn, 3)) if noise_gas is None else f64(noise_gas, (n_sn, 3))
    newpoints = pts[sp] + noise * d0
    newvels = vel[sp]
    out = (dust_comps, gas_release, gas_release, dust_mass, gas_masses, stars_mass, newpoints, newvels, np.zeros(n_sn),
           np.ones(n_dust) * 2, np.zeros(n_sn), np.zeros(n_dust), E[sp] / 2., sp, dustpoints, dustvels)
    return out + (dict(dust_len=dust_len),) if full else out


def row_means(f_un, mu_specie=None, gamma=None):
    """drv:393-394 -> (mu_array, gamma_array) = sum(f_un table, axis=1) / sum(f_un, axis=1)."""
    fun = f64(f_un)
    S = fun.shape[1]
    mus, gam = chem_table(S, mu_specie, "mu_specie"), chem_table(S, gamma, "gamma")
    tot = np.sum(fun, axis=1)
    return np.sum(fun * mus, axis=1) / tot, np.sum(fun * gam, axis=1) / tot


def supernova_insert(state, explosion, t_cmb=None, star_ages=None, sizes=None, d=None, m_0=None, mu_specie=None, gamma=None):
    """drv:363-382 and drv:393-394 on arrays -> a new state dict; `state` (particle_type, E_internal, f_un, mass,
    velocities, points, T) and `explosion` (supernova_explosion's tuple) are not modified.  In the driver's order: the
    star rows rewritten (E_internal, f_un, mass), the dust rows and then the gas rows appended, T extended by zeros and
    clamped as a whole (T[T < t_cmb] = t_cmb; a NaN stays), mu_array and gamma_array formed again for every row.
    star_ages is extended by -2 when given; sizes by the rule of drv:373-378 when sizes, d and m_0 are given.  total_accel
    keeps its old shape: the caller sees the mismatch the driver sees (drv:482-485).  With mean_grain_mass and mean_cross
    in the state, the rewritten and the new rows get theirs from grain_mass() and sigma_effective()."""
    (dust_comps, gas_comps, star_comps, dust_mass, gas_mass, stars_mass, newpoints, newvels, newgastype, newdusttype, new_eint_stars,
     new_eint_dust, new_eint_gas, sp, dustpoints, dustvels) = tuple(explosion)[:16]          # (full=True's dict is not read)
    sp = np.asarray(sp, dtype=np.int64).reshape(-1)
    tc = float(globals()["t_cmb"] if t_cmb is None else t_cmb)
    pt = np.concatenate((f64(state["particle_type"]), newdusttype, newgastype))           # drv:363
    E, fun, m = np.array(f64(state["E_internal"])), np.array(f64(state["f_un"])), np.array(f64(state["mass"]))
    n_old = m.shape[0]
    E[sp] = new_eint_stars
    fun[sp] = star_comps
    m[sp] = stars_mass
    E = np.concatenate((E, new_eint_dust, new_eint_gas))
    m = np.concatenate((m, dust_mass, gas_mass))
    fun = np.vstack([fun, dust_comps, gas_comps])
    vel = np.concatenate((f64(state["velocities"]), dustvels, newvels))
    pts = np.vstack([f64(state["points"]), dustpoints, newpoints])
    n = pts.shape[0]
    out = dict(state)
    if star_ages is not None:
        out["star_ages"] = np.concatenate((star_ages, np.ones(len(dustpoints)) * (-2), np.ones(len(sp)) * (-2)))
    if sizes is not None and d is not None and m_0 is not None:
        sz = np.zeros(n)
        sz[:n_old] = sizes
        new = (pt == 0) & (sz == 0)
        sz[new] = (m[new] / m_0) ** (1. / 3.) * d
        sz[(pt == 1) & (sz == 0)] = d / 10000.
        sz[(pt == 2) & (sz == 0)] = d
        out["sizes"] = sz
    T = np.zeros(n)
    T[:n_old] += f64(state["T"])
    T[T < tc] = tc
    mu, gam = row_means(fun, mu_specie, gamma)
    out.update(particle_type=pt, E_internal=E, f_un=fun, mass=m, velocities=vel, points=pts, T=T, mu_array=mu, gamma_array=gam)
    if state.get("mean_grain_mass") is not None and state.get("mean_cross") is not None:
        touched = np.concatenate((sp, np.arange(n_old, n)))
        mgm = np.concatenate((f64(state["mean_grain_mass"]), np.zeros(n - n_old)))
        mcs = np.concatenate((f64(state["mean_cross"]), np.zeros(n - n_old)))
        mgm[touched] = np.sum(grain_mass() * fun[touched], axis=1)
        mcs[touched] = np.sum(sigma_effective() * fun[touched], axis=1)
        out["mean_grain_mass"], out["mean_cross"] = mgm, mcs
    return out


# ==============================================================================================
# The adaptive length scale and sizes: the closing block of the time loop (drv:493-540)
# ==============================================================================================
SCALE_COUNTS = ("bonus", "capped", "nan_to_num", "missing")
SCALE_STAGES = ("keys", "select", "reverse_counts", "adapt", "write_back")


def _scale_result(n_slow, n_nan, lo, a, b, max_dist, d):
    return dict(n_slow=int(n_slow[0]), n_nan=int(n_nan[0]), lo=int(lo[0]), a=float(a[0]), b=float(b[0]),
                max_dist=float(max_dist[0]), d=float(d[0]))


def _scale_outputs():
    return [np.zeros(1, dtype=np.int64) for _ in range(3)] + [np.zeros(1) for _ in range(4)]


def length_scale(points, velocities, N_INT_PER_PARTICLE, q=90., v_max=80000., fill=0.9, full=False):
    """drv:493, 515-521 -> d, the driver's global length scale: from the q-th percentile (np.percentile, method linear) of
    |x|^2 over the rows slower than v_max and from their count (include/sphx.h sphx_length_scale).  The device finds the
    two order statistics the percentile interpolates between and the count; the result has np.percentile's bits.  No slow
    row: ValueError (np.percentile raises IndexError).  A NaN position among the slow rows gives NaN, as NumPy does.
    full=True -> dict: n_slow, n_nan, lo, a, b, max_dist, d."""
    pts = f64(points)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError("points must be (N, 3)")
    n = pts.shape[0]
    vel = f64(velocities, (n, 3))
    o = _scale_outputs()
    c_ = context()
    c_.check(c_.lib.sphx_length_scale(c_.h, n, dp(pts), dp(vel), float(v_max) ** 2, float(np.true_divide(q, 100)),
                                      float(N_INT_PER_PARTICLE), float(fill), ip(o[0]), ip(o[1]), ip(o[2]), dp(o[3]), dp(o[4]),
                                      dp(o[5]), dp(o[6])))
    res = _scale_result(*o)
    return res if full else res["d"]


def adapt_sizes(neighbor, densities, densities_0, sizes, particle_type, d, raise_factor, full=False):
    """drv:527-538 -> the new sizes (N,): the gas rows scaled by exp(-(rho - rho0) / (3 rho)) - plus 0.1 for a row that
    lists, and is listed by, almost nobody - and capped at d, the dust rows set to d / raise_factor**(1./3.), the stars
    left (include/sphx.h sphx_adapt_sizes).  densities_0 None, or of another length than densities (drv:532): the scale
    is 1.  An entry of the list outside [0, N) is ignored.  The given sizes are not modified; drv:540, densities_0 =
    densities, is the caller's.  full=True -> (sizes, dict: exp_neighbor_count, num_nontrivial (N,) int64, new_smoothing
    (N,), counts (SCALE_COUNTS))."""
    nb, n, k_ = _nk(neighbor)
    rho = f64(densities, (n,))
    rho0 = None
    if densities_0 is not None and len(densities_0) == n:
        rho0 = f64(densities_0, (n,))
    h, pt = f64(sizes, (n,)), f64(particle_type, (n,))
    d = float(d)
    d_dust = d / raise_factor ** (1. / 3.)                                         # drv:538
    out = np.zeros(n)
    rev = nt = sm = None
    if full:
        rev, nt, sm = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n)
    counts = np.zeros(len(SCALE_COUNTS), dtype=np.int64)
    c_ = context()
    c_.check(c_.lib.sphx_adapt_sizes(c_.h, n, k_, ip(nb), dp(rho), dp(rho0), dp(h), dp(pt), d, float(d_dust), dp(out), ip(rev), ip(nt),
                                     dp(sm), ip(counts)))
    if full:
        return out, dict(exp_neighbor_count=rev, num_nontrivial=nt, new_smoothing=sm,
                         counts=dict(zip(SCALE_COUNTS, (int(x) for x in counts))))
    return out


def scale_last_timing():
    """Device time of the last length_scale / adapt_sizes call of this module, from HIP events (include/sphx.h
    sphx_scale_last_timing) -> dict of ms: keys, select, reverse_counts, adapt, write_back."""
    return _last_timing("sphx_scale_last_timing", SCALE_STAGES)


# ==============================================================================================
# The census, the ordered selections and the stellar clock (drv:244, 339-342, 465-468, 604, 616-622, 636, 656-664)
# ==============================================================================================
CENSUS_FIXED = 13                # include/sphx.h sphx_census: the totals before the by-species ones
CENSUS_STAGES = ("prepare", "chunk_sums", "totals", "read_back")
AGB_WINDOW = (1., 7.)            # drv:660, solar masses


def _census_result(tot, counts, mx, S, have_dyn=True):
    """The dict of census() from the C call's outputs.  star_massfrac and star_numfrac as drv:616-617 forms them from the
    sums and counts, in NumPy's division: with no star or no non-dust row they are what NumPy gives (0, nan or inf)."""
    n_gas, n_star, n_dust, n_nondust = (int(v) for v in counts)
    out = dict(gas_mass=float(tot[0]), star_mass=float(tot[1]), dust_mass=float(tot[2]), nondust_mass=float(tot[3]),
               total_mass=float(tot[4]), n_gas=n_gas, n_star=n_star, n_dust=n_dust, n_nondust=n_nondust,
               max_star_mass=float(mx) if n_star else None)
    with np.errstate(all="ignore"):
        out["star_massfrac"] = float(np.float64(tot[1]) / np.float64(tot[3]))
        out["star_numfrac"] = float(np.float64(n_star) / np.float64(n_nondust))
        out["net_accel"] = np.array(tot[5:8]) / np.float64(tot[4]) if have_dyn else None
    out["momentum"] = np.array(tot[8:11]) if have_dyn else None
    out["kinetic"] = 0.5 * float(tot[11]) if have_dyn else None
    out["internal"] = float(tot[12]) if have_dyn else None
    for q, nm in enumerate(("gas_mass_by_species", "star_mass_by_species", "dust_mass_by_species")):
        out[nm] = np.array(tot[CENSUS_FIXED + q * S:CENSUS_FIXED + (q + 1) * S]) if S else None
    return out


def census(mass, particle_type, f_un=None, mu_specie=None, velocities=None, total_accel=None, E_internal=None):
    """The sums, counts and the maximum the driver reports every pass and saves at the end (drv:341, 465-468, 616-617, 636,
    656-658), in one fused pass on the device (include/sphx.h sphx_census) -> dict: gas_mass, star_mass, dust_mass,
    nondust_mass, total_mass, n_gas, n_star, n_dust, n_nondust, max_star_mass (None without a star), star_massfrac,
    star_numfrac, and with f_un the (S,) arrays gas_, star_ and dust_mass_by_species (else None); net_accel, momentum,
    kinetic and internal are formed from velocities, total_accel and E_internal (a missing array counts as zeros; all three
    missing: None).  Every sum runs over the particle index in the order of the library's ordered totals: the same bits on
    every call.  A row outside a sum's mask does not enter it, NaN or not."""
    m = f64(mass).reshape(-1)
    n = m.shape[0]
    pt = f64(particle_type, (n,))
    fu = mus = None
    S = 0
    if f_un is not None:
        fu = f64(f_un)
        if fu.ndim != 2 or fu.shape[0] != n:
            raise ValueError("f_un must be (N, S)")
        S = fu.shape[1]
        mus = chem_table(S, mu_specie, "mu_specie")
    vel = None if velocities is None else f64(velocities, (n, 3))
    acc = None if total_accel is None else f64(total_accel, (n, 3))
    E = None if E_internal is None else f64(E_internal, (n,))
    tot = np.zeros(CENSUS_FIXED + 3 * S); counts = np.zeros(4, dtype=np.int64); mx = np.zeros(1)
    c_ = context()
    c_.check(c_.lib.sphx_census(c_.h, n, S, dp(m), dp(pt), dp(fu), dp(mus), dp(vel), dp(acc), dp(E), dp(tot), ip(counts), dp(mx)))
    return _census_result(tot, counts, mx[0], S, have_dyn=not (vel is None and acc is None and E is None))


def census_last_timing():
    """Device time of the last census() of this module from HIP events -> dict of ms (CENSUS_STAGES)."""
    return _last_timing("sphx_census_last_timing", CENSUS_STAGES)


def _select_outputs(cap, S):
    cap = max(int(cap), 1)
    return (np.zeros(1, dtype=np.int64), np.zeros(cap, dtype=np.int64), np.zeros(cap), np.zeros(cap), np.zeros(cap),
            np.zeros((cap, S)) if S else None)


def _select_result(o):
    cnt = int(o[0][0])
    return dict(ids=o[1][:cnt].copy(), mass=o[2][:cnt].copy(), T=o[3][:cnt].copy(), star_ages=o[4][:cnt].copy(),
                f_un=None if o[5] is None else o[5][:cnt].copy())


def select_rows(mass, particle_type, ptype, T=None, star_ages=None, f_un=None, window=None):
    """The rows with particle_type == ptype - with window = (lo, hi) also lo < mass / solar_mass < hi (drv:660) - in
    ascending particle index, selected and compacted on the device (include/sphx.h sphx_census_select) -> dict: ids, mass,
    T, star_ages (zeros where the array is not given), f_un (rows, or None)."""
    m = f64(mass).reshape(-1)
    n = m.shape[0]
    pt = f64(particle_type, (n,))
    Tt = None if T is None else f64(T, (n,))
    ag = None if star_ages is None else f64(star_ages, (n,))
    fu = None if f_un is None else f64(f_un)
    S = 0 if fu is None else fu.shape[1]
    cap = int(np.count_nonzero(pt == ptype))
    o = _select_outputs(cap, S)
    lo, hi = (0., 0.) if window is None else window
    c_ = context()
    c_.check(c_.lib.sphx_census_select(c_.h, n, S, dp(m), dp(pt), dp(Tt), dp(ag), dp(fu), int(ptype), 0 if window is None else 1,
                                       float(solar_mass), float(lo), float(hi), cap, ip(o[0]), ip(o[1]), dp(o[2]), dp(o[3]), dp(o[4]),
                                       dp(o[5])))
    return _select_result(o)


def advance_star_ages(star_ages, particle_type, dt):
    """drv:604 -> the new star_ages: ages[(particle_type == 1) & (ages > -2)] += dt (include/sphx.h
    sphx_advance_star_ages).  The given array is not modified."""
    a = np.array(f64(star_ages).reshape(-1))
    n = a.shape[0]
    pt = f64(particle_type, (n,))
    c_ = context()
    c_.check(c_.lib.sphx_advance_star_ages(c_.h, n, dp(a), dp(pt), float(dt)))
    return a


def _schedule_of(rows):
    """drv:244, 339-341 on the compacted star rows (ids ascending, mass, star_ages): the reference's own expression, on the
    host, so the comparison with 1 has the reference's bits."""
    ids, m, ages = rows["ids"], rows["mass"], rows["star_ages"]
    if ids.shape[0] == 0:                # drv:243: the block is skipped without a star
        return dict(supernova_pos=np.zeros(0, dtype=np.int64), max_rel_age=None, max_star_mass=None, n_star=0)
    with np.errstate(all="ignore"):
        rel = ages / luminosity_relation(m / solar_mass, lifetime=1) / (year * 1e10)
        return dict(supernova_pos=ids[rel > 1.], max_rel_age=float(np.max(rel)), max_star_mass=float(np.max(m / solar_mass)),
                    n_star=int(ids.shape[0]))


def supernova_schedule(star_ages, particle_type, mass):
    """drv:244, 339-342 -> dict: supernova_pos (ascending indices of the stars whose age exceeds their lifetime),
    max_rel_age and max_star_mass (solar masses) over the stars, n_star.  The device selects the star rows; the ratio and
    its comparison are the reference's NumPy expression on those rows.  Gas rows (age -1) and inserted rows (-2) can never
    pass the test, so leaving them out changes nothing in supernova_pos; max_rel_age is the reference's whenever a star's
    relative age is the largest (ages of stars are >= 0).  Without a star: an empty supernova_pos, None for the maxima."""
    return _schedule_of(select_rows(mass, particle_type, 1, star_ages=star_ages))


def _agb_outputs(n, rows, OVERALL_AGE, mus):
    """drv:660-664 from the compacted AGB rows, with the driver's own expressions."""
    ids, m, ages, fu = rows["ids"], rows["mass"], rows["star_ages"], rows["f_un"]
    cond = np.zeros(n, dtype=bool)
    cond[ids] = True
    fm = fu * mus
    with np.errstate(all="ignore"):
        return dict(AGB_condition=cond, AGB_list=m,
                    AGB_time_until=luminosity_relation(m / solar_mass, lifetime=1) * 1e10 * year - ages + OVERALL_AGE,
                    AGB_metallicity=np.sum(fm.T[6:], axis=0) / np.sum(fm, axis=1),
                    AGB_composition=(fm.T / np.sum(fm, axis=1)).T)


def run_outputs(mass, particle_type, f_un, star_ages, OVERALL_AGE, mu_specie=None):
    """The entries of the driver's closing np.savez (drv:670) that depend on the state -> dict: gas_, star_ and
    dust_mass_by_species (drv:656-658, from census()), AGB_condition, AGB_list, AGB_time_until, AGB_metallicity and
    AGB_composition (drv:660-664, from the AGB rows the device selects, with the driver's expressions)."""
    fu = f64(f_un)
    S = fu.shape[1]
    mus = chem_table(S, mu_specie, "mu_specie")
    cen = census(mass, particle_type, fu, mus)
    out = {nm: cen[nm] for nm in ("gas_mass_by_species", "star_mass_by_species", "dust_mass_by_species")}
    rows = select_rows(mass, particle_type, 1, star_ages=star_ages, f_un=fu, window=AGB_WINDOW)
    out.update(_agb_outputs(fu.shape[0], rows, OVERALL_AGE, mus))
    return out


# ==============================================================================================
# The projected maps: the state integrated along a line of sight onto a pixel grid (drv:563-597 draws the cloud each pass)
# ==============================================================================================
MAP_FIELDS = ("gas_column", "dust_column", "gas_temperature", "dust_temperature", "count")
MAP_STAGES = ("footprints", "count_scan", "list_build", "tiles", "read_back")


def _map_args(axes, center, half_width, npix, depth, fields):
    """The image's arguments as the C calls take them, and the zeroed (n_v, n_u) outputs of the fields asked for."""
    ax = np.ascontiguousarray(np.asarray(axes, dtype=np.int32).reshape(-1))
    np_ = np.ascontiguousarray(np.broadcast_to(np.asarray(npix, dtype=np.int32), (2,)))
    ce = np.ascontiguousarray(np.broadcast_to(np.asarray(center, dtype=np.float64), (2,)))
    hw = np.ascontiguousarray(np.broadcast_to(np.asarray(half_width, dtype=np.float64), (2,)))
    if ax.shape != (2,):
        raise ValueError("axes must be two coordinate indices")
    dep = None if depth is None else f64(depth, (2,))
    for f in fields:
        if f not in MAP_FIELDS:
            raise ValueError("unknown field %r (one of %s)" % (f, ", ".join(MAP_FIELDS)))
    if int(np_[0]) * int(np_[1]) > 1 << 28:       # (the C call's own limit, before the outputs are allocated)
        raise ValueError("npix: %d x %d pixels (at most 2^28)" % (np_[0], np_[1]))
    shape = (max(int(np_[1]), 0), max(int(np_[0]), 0))
    out = {f: np.zeros(shape, dtype=np.int64 if f == "count" else np.float64) for f in MAP_FIELDS if f in fields}
    return ax, ce, hw, np_, dep, out


def _map_call(fn, head, geom, out):
    """One of the two C calls: head are its arguments in front of the image's -> the dict of project_maps."""
    ax, ce, hw, np_, dep = geom
    sk, pr = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64)
    c32 = lambda a: a.ctypes.data_as(_lib.c_int32_p)
    rc = fn(*head, c32(ax), dp(ce), dp(hw), c32(np_), dp(dep), *[dp(out.get(f)) for f in MAP_FIELDS[:4]], ip(out.get("count")),
            ip(sk), ip(pr))
    res = dict(out)
    res["skipped"], res["pairs"] = int(sk[0]), int(pr[0])
    return rc, res


def project_maps(points, mass, particle_type, sizes, T, d, axes=(1, 2), center=(0, 0), half_width=1.0, npix=256, depth=None,
                 fields=MAP_FIELDS):
    """The particles integrated along a coordinate axis onto a pixel grid (include/sphx.h sphx_project_maps) -> dict of
    (n_v, n_u) arrays - gas_column and dust_column [kg/m^2], gas_temperature and dust_temperature (column-weighted, 0 where
    there is nothing), count (int64: particles over the pixel) - of the `fields` asked for, plus skipped (gas and dust rows
    that are not finite or have no positive radius) and pairs ((particle, 16 x 16 tile) pairs listed).  axes = (a_u, a_v):
    the image's horizontal and vertical coordinate, the line of sight is the third; center, half_width and npix: a pair
    (u, v) or one value for both; depth = (lo, hi): only particles with lo <= line-of-sight coordinate < hi.  Gas has the
    footprint h(m) = (m/m_0)^(1/3) d, dust its sizes; stars have none.  Values are at pixel centres, every sum in ascending
    particle index: the same bits on every call."""
    pts = f64(points)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError("points must be (N, 3)")
    n = pts.shape[0]
    m, pt, sz, Tt = f64(mass).reshape(-1), f64(particle_type, (n,)), f64(sizes, (n,)), f64(T, (n,))
    if m.shape != (n,):
        raise ValueError("mass must be (N,)")
    *geom, out = _map_args(axes, center, half_width, npix, depth, fields)
    c_ = context()
    rc, res = _map_call(c_.lib.sphx_project_maps, (c_.h, n, dp(pts), dp(m), dp(pt), dp(sz), dp(Tt), float(d)), geom, out)
    c_.check(rc)
    return res


def map_last_timing():
    """Device time of the last project_maps() of this module from HIP events -> dict of ms (MAP_STAGES)."""
    return _last_timing("sphx_map_last_timing", MAP_STAGES)
