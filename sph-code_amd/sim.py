"""Device-resident step loop: the fused hot path of sph/code_running.py:217-491
(search -> dt -> density/pressure/viscosity sums -> leapfrog), nothing leaves HBM between steps.

State in, state out keeps the reference's array conventions (sph/code_running.py:114-177):
points/velocities (N,3), mass, particle_type (f64 0/1/2), f_un (N,S), T, mu_array,
gamma_array, E_internal, total_accel.
"""
import ctypes as C
import logging

import numpy as np

from . import _lib
from ._lib import dp, f64
from .compat import ARB_FIELDS, rad_mode_code, visc_mode_code

log = logging.getLogger("sph_code_amd")


class Simulation:
    def __init__(self, state, n_neigh=40, dist=None, device=None, with_species=False, ctx=None,
                 incremental=False, with_drag=False, gravity=None, G=6.67430e-11, clip_grad=False,
                 forms="hydro_update", d=None, gravity_order=2, agb=None, visc_mode="ref_axis0", star_ages=None):
        """with_species: carry f_un on the device; every step (hydro_update mode) then also forms the species number
        densities F[s,i] of nsc:624-627 on its own neighbour list.  agb = (splines, mapto, divisor) as
        sph_code_amd.agb.interpolate_amounts returns them: the same pass also leaves the per-particle metallicity
        (the expression of code_running.py:663) and the AGB dust yields of config_helper.py:183-189 (download_species).
        visc_mode="pairwise": the per-pair viscosity of include/sphx.h sphx_set_visc_mode (hydro_update mode only; the
        loop forms' viscosity is pairwise already)."""
        vmode = visc_mode_code(visc_mode)
        if vmode and forms == "loop":
            raise ValueError("visc_mode='pairwise' is for forms='hydro_update': the loop forms' viscosity is pairwise already")
        if agb is not None and with_species and state.get("f_un") is not None:
            from . import compat
            if np.shape(state["f_un"])[-1] > len(compat.mu_specie):      # the C call reads one molecular weight per species
                raise ValueError("agb: the state carries %d species, mu_specie has %d entries"
                                 % (np.shape(state["f_un"])[-1], len(compat.mu_specie)))
        self.ctx = ctx if ctx is not None else _lib.Context(device)
        self.ctx.set_incremental(incremental)
        self.k = int(n_neigh)
        self.dist = 0.0 if dist is None or not np.isfinite(dist) else float(dist)
        self.first = True
        self._phase_ran = False          # a dust_phase has rewritten mass, f_un, mu_array, gamma_array on the device
        self._with_drag = bool(with_drag)
        pts = f64(state["points"])
        n = pts.shape[0]
        self.n = n
        self._ptype = f64(state["particle_type"], (n,)).copy()
        vel = f64(state["velocities"], (n, 3))
        fu = f64(state["f_un"]) if (with_species and state.get("f_un") is not None) else None
        acc = state.get("total_accel")
        acc = f64(acc, (n, 3)) if acc is not None else None
        c = self.ctx
        c.check(c.lib.sphx_state_upload(
            c.h, n, 0 if fu is None else fu.shape[1], dp(pts), dp(vel), dp(f64(state["mass"], (n,))),
            dp(f64(state["particle_type"], (n,))), dp(fu), dp(f64(state["T"], (n,))),
            dp(f64(state["mu_array"], (n,))), dp(f64(state["gamma_array"], (n,))),
            dp(f64(state["E_internal"], (n,))), dp(acc)))
        c.check(c.lib.sphx_set_clip_grad(c.h, 1 if clip_grad else 0))
        c.check(c.lib.sphx_set_visc_mode(c.h, vmode))
        if forms not in ("hydro_update", "loop"):
            raise ValueError("forms must be 'hydro_update' or 'loop'")
        if forms == "loop":            # the reference's time loop: nsc.density, del_pressure, ... with the global d
            if d is None:
                raise ValueError("forms='loop' needs the driver's global d (code_running.py:67-68)")
            c.check(c.lib.sphx_state_set_loop_forms(c.h, 1, float(d)))
        if gravity is not None:
            if gravity not in ("direct", "tree"):
                raise ValueError("gravity must be None, 'direct' or 'tree'")
            c.check(c.lib.sphx_state_set_gravity(c.h, 1 if gravity == "direct" else 2, float(G)))
            # tree: cells carry their second moments (order 2, ~0.1 % rms force error) or monopoles only (1, ~1 %)
            c.check(c.lib.sphx_set_gravity_order(c.h, int(gravity_order)))
        self.n_species = 0 if fu is None else fu.shape[1]
        if agb is not None:
            if fu is None:
                raise ValueError("agb needs with_species=True and a state with f_un")
            from . import compat
            splines, mapto, divisor = agb
            i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
            ntx = i32([sp.get_knots()[0].size for sp in splines]); nty = i32([sp.get_knots()[1].size for sp in splines])
            cat = lambda parts: np.ascontiguousarray(np.concatenate([np.asarray(q, dtype=np.float64).ravel() for q in parts]))
            tx = cat([sp.get_knots()[0] for sp in splines]); ty = cat([sp.get_knots()[1] for sp in splines])
            cf = cat([sp.get_coeffs() for sp in splines]); mp = i32(mapto)
            mu = np.ascontiguousarray(compat.mu_specie[:self.n_species], dtype=np.float64)
            p32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
            c.check(c.lib.sphx_state_set_agb(c.h, len(splines), p32(ntx), p32(nty), dp(tx), dp(ty), dp(cf), p32(mp),
                                             float(divisor), dp(mu), compat.solar_mass))
        self.has_agb = agb is not None
        if with_drag:
            # per-particle mean grain mass / cross-section as nsc.net_impulse forms them (nsc:720-726)
            from . import compat
            fu_all = f64(state["f_un"])
            mgm = np.ascontiguousarray(np.sum(compat.grain_mass() * fu_all, axis=1))
            mcs = np.ascontiguousarray(np.sum(compat.sigma_effective() * fu_all, axis=1))
            c.check(c.lib.sphx_state_set_drag(c.h, dp(mgm), dp(mcs)))
        self._has_ages = False
        if star_ages is not None:
            self.set_star_ages(star_ages)

    def step(self, nsteps=1, fixed_dt=0.0):
        c = self.ctx
        c.check(c.lib.sphx_step(c.h, int(nsteps), self.k, self.dist, 1 if self.first else 0, float(fixed_dt)))
        self.first = False
        self._log_failures()

    FAILURE_COUNTERS = ("bad_accel", "bad_energy", "bad_state", "bad_h", "short_rows")

    def failures(self):
        """-> dict of the library's failure counters (include/sphx.h sphx_stats: particles whose acceleration / energy /
        updated state / kNN radius was NaN, inf or 0 before the reference's nan_to_num guards, drv:233-238,460-463,490;
        searches that gave up short), summed since the last reset_stats().  All zero in a sane run."""
        st = self.ctx.stats()
        return {k_: int(st[k_]) for k_ in self.FAILURE_COUNTERS}

    def _log_failures(self):
        f = self.failures()
        seen = getattr(self, "_failures_seen", None) or dict.fromkeys(self.FAILURE_COUNTERS, 0)
        new = {k_: f[k_] - seen.get(k_, 0) for k_ in f if f[k_] > seen.get(k_, 0)}
        self._failures_seen = f
        if new:
            log.warning("sphx step: non-finite values met (particles): %s  [cumulative: %s]", new, f)

    def download(self):
        n = self.n
        out = dict(points=np.empty((n, 3)), velocities=np.empty((n, 3)), total_accel=np.empty((n, 3)),
                   E_internal=np.empty(n), T=np.empty(n), sizes=np.empty(n), densities=np.empty(n),
                   num_densities=np.empty(n), visc_heat=np.empty(n))
        dt = C.c_double(0.0)
        c = self.ctx
        c.check(c.lib.sphx_state_download(
            c.h, dp(out["points"]), dp(out["velocities"]), dp(out["total_accel"]), dp(out["E_internal"]),
            dp(out["T"]), dp(out["sizes"]), dp(out["densities"]), dp(out["num_densities"]),
            dp(out["visc_heat"]), C.cast(C.byref(dt), _lib.c_double_p)))
        out["dt"] = dt.value
        # P_i = n_i k_B T_i with n and T of the instant the last step's sums were formed at (the reference forms it and
        # drops it, nsc:608; out["T"] is the temperature AFTER the update, drv:491 - not the one n_i belongs to)
        out["pressure"] = np.empty(n)
        c.check(c.lib.sphx_state_download_pressure(c.h, dp(out["pressure"])))
        return out

    SAMPLE_FIELDS = ARB_FIELDS

    def sample(self, arb_points, d, fields=("density", "dust_density", "temperature", "dust_temperature"),
               n_part=None, value=None, radius=0.0, with_stats=False):
        """The fields of nsc:1428-1527 at arbitrary points, from the state as it is on the device (include/sphx.h
        sphx_state_sample; after the first step).  arb_points (..., 3) -> dict of arrays of shape (...): a (H, W, 3)
        slice gives images.  d: the driver's global d (drv:68).  "photoionization" needs n_part and value, (N,) in the
        particle order of the uploaded state.  radius <= 0: the ball radius is max(sizes).  The step loop is not
        disturbed.  with_stats: also "count" (...) int64 and "candidates".
        "temperature" and "photoionization" count a particle only inside its own support (include/sphx.h
        sphx_arb_fields): nothing else for T >= 0.  A particle with T < 0 drops out of "temperature" (the result
        is the reference's formula on max(T, 0)) - and forms="hydro_update" leaves negative temperatures behind from the
        second step on; forms="loop" keeps T positive."""
        q = f64(arb_points)
        if q.ndim < 1 or q.shape[-1] != 3:
            raise ValueError("arb_points must be (..., 3)")
        shape = q.shape[:-1]
        q = np.ascontiguousarray(q.reshape(-1, 3))
        m = q.shape[0]
        for f in fields:
            if f not in self.SAMPLE_FIELDS:
                raise ValueError("unknown field %r (one of %s)" % (f, ", ".join(self.SAMPLE_FIELDS)))
        if "photoionization" in fields and (n_part is None or value is None):
            raise ValueError("field 'photoionization' needs n_part and value")
        npart = None if n_part is None else f64(n_part, (self.n,))
        val = None if value is None else f64(value, (self.n,))
        out = {f: np.zeros(m) for f in fields}
        cnt = np.zeros(m, np.int64) if with_stats else None
        cand = np.zeros(1, np.int64)
        c = self.ctx
        c.check(c.lib.sphx_state_sample(c.h, float(d), dp(npart), dp(val), m, dp(q), float(radius),
                                        *[dp(out.get(f)) for f in self.SAMPLE_FIELDS], _lib.ip(cnt), _lib.ip(cand)))
        out = {f: a.reshape(shape) for f, a in out.items()}
        if with_stats:
            out["count"] = cnt.reshape(shape)
            out["candidates"] = int(cand[0])
        return out

    def sample_timing(self):
        """Device time of the last sample() from HIP events -> dict of ms: upload, build, kernels, download."""
        ms = np.zeros(4)
        c = self.ctx
        c.check(c.lib.sphx_arb_last_timing(c.h, dp(ms)))
        return dict(zip(("upload", "build", "kernels", "download"), ms.tolist()))

    def rad_transfer(self, sources, luminosities, targets, cross_array, dt, mode="line", full=False):
        """Lines 922-965 of nsc.rad_heating on the state as it is on the device (include/sphx.h
        sphx_state_rad_transfer; after the first step) -> (lf2 (G,), momentum (G,3), extinction (G,)) over the G non-star
        particles in the order of the uploaded state; full=True: also blocked, star_distance, lum_factor.  The bits are
        those of compat.rad_transfer on the downloaded state.  cross_array (N,) in the particle order of the uploaded
        state.  The step loop is not disturbed."""
        code = rad_mode_code(mode)
        src = np.ascontiguousarray(f64(sources).reshape(-1, 3))
        dst = np.ascontiguousarray(f64(targets).reshape(-1, 3))
        L = f64(luminosities).reshape(-1)
        if L.shape[0] != src.shape[0]:
            raise ValueError("luminosities must have one entry per source")
        cr = f64(cross_array, (self.n,))
        if not hasattr(self, "_n_gas"):
            self._n_gas = int(np.count_nonzero(self._ptype != 1))
        G = self._n_gas
        out = [np.zeros(G), np.zeros((G, 3)), np.zeros(G)]
        extra = [np.zeros((src.shape[0], dst.shape[0])), np.zeros((src.shape[0], dst.shape[0])),
                 np.zeros((src.shape[0], G))] if full else [None, None, None]
        c = self.ctx
        c.check(c.lib.sphx_state_rad_transfer(c.h, dp(cr), src.shape[0], dp(src), dp(L), dst.shape[0], dp(dst), float(dt), code,
                                              *[dp(a) for a in out + extra]))
        return tuple(out + extra) if full else tuple(out)

    def rad_timing(self):
        """Device time of the last rad_transfer() from HIP events -> dict of ms: upload, columns, deposit, download."""
        ms = np.zeros(4)
        c = self.ctx
        c.check(c.lib.sphx_rad_last_timing(c.h, dp(ms)))
        return dict(zip(("upload", "columns", "deposit", "download"), ms.tolist()))

    def download_species(self):
        """-> dict: f_un_neighbor (S,N) as nsc.hydro_update returns it (nsc:671), and with an AGB table also
        metallicity (N,) and agb_dust (N,S)."""
        n, S = self.n, self.n_species
        if S < 1:
            raise RuntimeError("the simulation carries no composition (with_species=True and a state with f_un)")
        out = dict(f_un_neighbor=np.empty((S, n)))
        Z = A = None
        if self.has_agb:
            out["metallicity"] = Z = np.empty(n)
            out["agb_dust"] = A = np.empty((n, S))
        c = self.ctx
        c.check(c.lib.sphx_state_download_species(c.h, dp(out["f_un_neighbor"]), dp(Z), dp(A)))
        return out

    # ---- the dust phase of the time loop (code_running.py:399-435) on the resident state ----------------------------
    def neighbors(self):
        """The last step's neighbour list -> (N, K) int64 in the particle order of the uploaded state, a missing entry N
        (compat.neighbors' convention).  It is the list of the positions the step started from: the driver's `neighbor`
        at drv:407.  After the first step; not with incremental=True."""
        out = np.empty((self.n, self.k), dtype=np.int64)
        c = self.ctx
        c.check(c.lib.sphx_state_download_neighbors(c.h, _lib.ip(out)))
        return out

    def download_composition(self):
        """-> dict: mass (N,), mu_array (N,), gamma_array (N,) and, with with_species=True, f_un (N,S), as they are on the
        device (a dust_phase rewrites them)."""
        n, S = self.n, self.n_species
        out = dict(mass=np.empty(n), mu_array=np.empty(n), gamma_array=np.empty(n))
        fu = None
        if S > 0:
            out["f_un"] = fu = np.empty((n, S))
        c = self.ctx
        c.check(c.lib.sphx_state_download_composition(c.h, dp(out["mass"]), dp(fu), dp(out["mu_array"]), dp(out["gamma_array"])))
        return out

    def download_drag(self):
        """-> (mean_grain_mass (N,), mean_cross (N,)) as the drag pass reads them (with_drag=True)."""
        mgm, mcs = np.empty(self.n), np.empty(self.n)
        c = self.ctx
        c.check(c.lib.sphx_state_download_drag(c.h, dp(mgm), dp(mcs)))
        return mgm, mcs

    def _d_or_remembered(self, d):
        if d is not None:
            return d
        if getattr(self, "_scale_d", None) is None:
            raise ValueError("d=None needs a length_scale() before it: there is no remembered d")
        return self._scale_d

    def dust_phase(self, dt, d, guard="count", full=False, **tables):
        """code_running.py:399-435 on the state as it is on the device (include/sphx.h sphx_state_dust_phase): f_un
        normalised, the loop-form density, chemisputtering_2, supernova_destruction on its outputs, and the bookkeeping
        that folds both into mass, f_un, mu_array and gamma_array - which the next step then reads.  The list is the last
        step's own (neighbors()), sizes the step's radii.  -> dict of the totals the driver prints (compat.PHASE_TOTALS,
        compat.PHASE_COUNTS) plus chem_counts and dust_counts; full=True adds the stage outputs density, mass_chem,
        f_un_chem, frac_destruction, frac_reuptake in the particle order of the uploaded state.  dt and d are the
        driver's; **tables as compat.dust_phase takes them (mu_specie, gamma, mineral_densities, sputtering_yields,
        mrn_constants, crit_mass, critical_density, species_curve), by default the module's.  With with_drag=True the
        per-particle drag coefficients are formed again from the new f_un (compat.grain_mass(), compat.sigma_effective()).
        The bits are those of compat.dust_phase on the downloaded state.  Needs with_species=True and one step."""
        from . import compat
        n = self.n
        d = self._d_or_remembered(d)     # (None: the d of the last length_scale())
        # (a state without a composition: the library refuses the call; the tables are sized by themselves)
        S = self.n_species or int(np.shape(tables["mu_specie"] if tables.get("mu_specie") is not None else compat.mu_specie)[0])
        t = compat.phase_tables(S, dt=dt, guard=guard, **tables)
        gm = se = None
        if self._with_drag:              # (the tables Simulation formed the coefficients from at upload)
            gm = np.ascontiguousarray(compat.grain_mass(), dtype=np.float64)
            se = np.ascontiguousarray(compat.sigma_effective(), dtype=np.float64)
            if gm.shape != (S,) or se.shape != (S,):
                raise ValueError("with_drag: grain_mass and sigma_effective hold %d species, the state %d" % (gm.shape[0], S))
        st = dict(density=np.empty(n), mass_chem=np.empty(n), f_un_chem=np.empty((n, S)), frac_destruction=np.empty((n, S)),
                  frac_reuptake=np.empty((n, S))) if full else {}
        cc = np.zeros(len(compat.CHEM_COUNTS), dtype=np.int64); dc = np.zeros(len(compat.DUST_COUNTS), dtype=np.int64)
        tot = np.zeros(len(compat.PHASE_TOTALS)); bc = np.zeros(len(compat.PHASE_COUNTS), dtype=np.int64)
        kv, kc, ks = t["knots"]
        c = self.ctx
        c.check(c.lib.sphx_state_dust_phase(
            c.h, t["dt"], float(d), dp(t["mu_specie"]), dp(t["gamma"]), dp(t["mineral_densities"]), dp(t["sputtering_yields"]),
            dp(t["mrn"]), float(compat.k), float(compat.amu), float(compat.m_0), t["crit_mass"], t["critical_density"],
            t["species_curve"].ctypes.data_as(_lib.c_int32_p), dp(kv), dp(kc), dp(ks), t["guard"], dp(gm), dp(se),
            dp(st.get("density")), dp(st.get("mass_chem")), dp(st.get("f_un_chem")), dp(st.get("frac_destruction")),
            dp(st.get("frac_reuptake")), _lib.ip(cc), _lib.ip(dc), dp(tot), _lib.ip(bc)))
        self._phase_ran = True
        out = dict(zip(compat.PHASE_TOTALS, (float(v) for v in tot)))
        out.update(zip(compat.PHASE_COUNTS, (int(v) for v in bc)))
        out["chem_counts"] = dict(zip(compat.CHEM_COUNTS, (int(v) for v in cc)))
        out["dust_counts"] = dict(zip(compat.DUST_COUNTS, (int(v) for v in dc)))
        out.update(st)
        return out

    def phase_timing(self):
        """Device time of the last dust_phase() from HIP events -> dict of ms: gather, density, chem, dust, bookkeeping."""
        ms = np.zeros(5)
        c = self.ctx
        c.check(c.lib.sphx_phase_last_timing(c.h, dp(ms)))
        return dict(zip(("gather", "density", "chem", "dust", "bookkeeping"), ms.tolist()))

    # ---- the radiative block of the time loop (code_running.py:247-316) on the resident state ------------------------
    RADPHASE_STAGES = ("cross_array", "lf2", "momentum", "extinction", "f_un_ionised", "frac_destroyed", "mu_heat", "gamma_heat",
                       "cross_heat", "E_heat", "T_heat", "energy", "rec_array", "cross_array_out")

    def rad_phase(self, dt, d, source_ids, luminosities, target_ids, frac_dest, photons_per_joule, t_max, cooling_timescale,
                  mode="line", full=False, t_cmb=None, mu_specie=None, gamma=None, cross_sections=None, driver_cross=None):
        """code_running.py:247-316 with N_RADIATIVE = 1 on the state as it is on the device (include/sphx.h
        sphx_state_rad_phase): rad_transfer, the photoionisation chemistry, the heating's bookkeeping, rad_cooling on the
        last step's own list, the cooling's bookkeeping - and f_un, mu_array, gamma_array, E_internal, T and the velocities
        written where the next step() and dust_phase() read them.  source_ids, luminosities, target_ids as compat.rad_setup
        returns them (particle indices of the uploaded state), frac_dest and photons_per_joule as compat.stellar_spectrum
        does; t_max and cooling_timescale are undefined in the driver and have no default; the tables as compat.rad_phase
        takes them.  -> dict of totals (compat.rad_phase's: skipped, E_before, E_after_heating, E_after_cooling, the clamp
        counts); full=True adds every stage's output (RADPHASE_STAGES) in the particle order of the uploaded state.  With
        no star the driver skips the block: {"skipped": True}, nothing written.  With with_drag=True the drag coefficients
        are formed again from the new f_un.  The bits are those of compat.rad_phase on the downloaded state and
        neighbors().  Needs with_species=True and one step."""
        from . import compat
        n = self.n
        d = self._d_or_remembered(d)     # (None: the d of the last length_scale())
        S = self.n_species or int(np.shape(mu_specie if mu_specie is not None else compat.mu_specie)[0])
        code = rad_mode_code(mode)
        mus, gam = compat.chem_table(S, mu_specie, "mu_specie"), compat.chem_table(S, gamma, "gamma")
        cs = compat.chem_table(S, cross_sections, "cross_sections")
        csd = compat.driver_cross_sections(S) if driver_cross is None else compat.chem_table(S, driver_cross, "cross_sections")
        fd = f64(frac_dest, (S,))
        src = np.ascontiguousarray(np.asarray(source_ids, dtype=np.int64).reshape(-1))
        dst = np.ascontiguousarray(np.asarray(target_ids, dtype=np.int64).reshape(-1))
        L = f64(luminosities).reshape(-1)
        if L.shape[0] != src.shape[0]:
            raise ValueError("luminosities must have one entry per source")
        gm = se = None
        if self._with_drag:
            gm = np.ascontiguousarray(compat.grain_mass(), dtype=np.float64)
            se = np.ascontiguousarray(compat.sigma_effective(), dtype=np.float64)
            if gm.shape != (S,) or se.shape != (S,):
                raise ValueError("with_drag: grain_mass and sigma_effective hold %d species, the state %d" % (gm.shape[0], S))
        if not hasattr(self, "_n_gas"):
            self._n_gas = int(np.count_nonzero(self._ptype != 1))
        G = self._n_gas
        st = {}
        heat = None
        if full:
            st = dict(cross_array=np.zeros(n), lf2=np.zeros(G), momentum=np.zeros((G, 3)), extinction=np.zeros(G),
                      f_un_ionised=np.zeros((n, S)), frac_destroyed=np.zeros((G, 3)), energy=np.zeros(n), rec_array=np.zeros((S, n)),
                      cross_array_out=np.zeros(n))
            heat = np.zeros((5, n))
        tot = np.zeros(3); cnt = np.zeros(8, dtype=np.int64); ng = np.zeros(1, dtype=np.int64)
        skipped = C.c_int(0)
        c = self.ctx
        # the physics stages read these from the context, as compat's array calls set them on theirs
        c.set_constants(k_B=compat.k, amu=compat.amu, m_h=compat.m_h, m_0=compat.m_0, solar_luminosity=compat.solar_luminosity, c=compat.c)
        c.check(c.lib.sphx_state_rad_phase(
            c.h, float(dt), float(d), src.shape[0], _lib.ip(src), dp(L), dst.shape[0], _lib.ip(dst), dp(fd), float(photons_per_joule),
            dp(mus), dp(gam), dp(cs), dp(csd), float(compat.amu), float(compat.t_cmb if t_cmb is None else t_cmb), float(t_max),
            float(cooling_timescale), float(compat.sb), float(compat.k), float(compat.m_h), code, dp(gm), dp(se),
            dp(st.get("cross_array")), dp(st.get("lf2")), dp(st.get("momentum")), dp(st.get("extinction")), dp(st.get("f_un_ionised")),
            dp(st.get("frac_destroyed")), dp(heat), dp(st.get("energy")), dp(st.get("rec_array")), dp(st.get("cross_array_out")),
            dp(tot), _lib.ip(cnt), _lib.ip(ng), C.byref(skipped)))
        if skipped.value:
            return dict(skipped=True)
        if int(ng[0]) != G:
            raise RuntimeError("the state holds %d non-star particles, the uploaded particle_type %d" % (int(ng[0]), G))
        self._phase_ran = True
        out = dict(skipped=False, E_before=float(tot[0]), E_after_heating=float(tot[1]), E_after_cooling=float(tot[2]))
        for q, nm in enumerate(compat.RADPHASE_COUNTS):
            out["heat_" + nm], out["cool_" + nm] = int(cnt[q]), int(cnt[4 + q])
        if full:
            for q, nm in enumerate(("mu_heat", "gamma_heat", "cross_heat", "E_heat", "T_heat")):
                st[nm] = heat[q].copy()
            out.update(st)
        return out

    def radphase_timing(self):
        """Device time of the last rad_phase() from HIP events -> dict of ms: gather, transfer, ionise_heat, cooling,
        bookkeeping (the last with the write-back and the outputs coming back)."""
        ms = np.zeros(5)
        c = self.ctx
        c.check(c.lib.sphx_state_radphase_last_timing(c.h, dp(ms)))
        return dict(zip(("gather", "transfer", "ionise_heat", "cooling", "bookkeeping"), ms.tolist()))

    # ---- the supernova event of the time loop (code_running.py:350-358) on the resident state, N unchanged ----------
    def supernova_impulse(self, supernova_ids, dt_0=None, mass_displaced=None, supernova_energy=None):
        """code_running.py:350-358 on the state as it is on the device (include/sphx.h sphx_state_supernova_impulse): for
        every star of supernova_ids (particle indices of the uploaded state, in the driver's order) the kick of
        nsc.supernova_impulse added to the resident velocities, then ct = crossing_time on the last step's own list
        (neighbors()), the step's radii and the kicked velocities, and the event's time step min(dt_0 / 100, ct).
        -> dict: dt (what the caller hands to dust_phase and step(fixed_dt=...)), ct, selections (per star (d_vels,
        selected ids) as compat.supernova_impulse returns them), sel_count, true_mass, vel, counts (compat.SN_COUNTS).
        The bits are those of compat.supernova_impulses and compat.crossing_time on the downloaded state.  dt_0,
        mass_displaced and supernova_energy default to compat's.  An empty supernova_ids is a no-op: dt is None.  The
        insertion of the new particles (drv:361-396) changes N: supernova_explosion, below.  Needs one step; not with
        incremental=True."""
        import re
        from . import compat
        ids = np.ascontiguousarray(np.asarray(supernova_ids, dtype=np.int64).reshape(-1))
        n_sn = ids.shape[0]
        if n_sn == 0:
            return dict(dt=None, ct=None, selections=[], sel_count=np.zeros(0, dtype=np.int64), true_mass=np.zeros(0), vel=np.zeros(0),
                        counts=dict.fromkeys(compat.SN_COUNTS, 0))
        M = float(compat.mass_displaced if mass_displaced is None else mass_displaced)
        E = float(compat.supernova_energy if supernova_energy is None else supernova_energy) * compat.SN_KICK_FRACTION
        dt0 = float(compat.dt_0 if dt_0 is None else dt_0)
        most = int(np.count_nonzero(self._ptype == 0)) * n_sn
        cap = min(most, compat._SN_FIRST_CAP)
        c = self.ctx
        while True:
            sel_count = np.zeros(n_sn, dtype=np.int64)
            sel_ids = np.zeros(max(cap, 1), dtype=np.int64); d_vels = np.zeros((max(cap, 1), 3))
            true_mass = np.zeros(n_sn); vel = np.zeros(n_sn)
            counts = np.zeros(len(compat.SN_COUNTS), dtype=np.int64)
            ct = C.c_double(0.0); dt = C.c_double(0.0)
            rc = c.lib.sphx_state_supernova_impulse(c.h, n_sn, _lib.ip(ids), M, E, dt0, cap, _lib.ip(sel_count), _lib.ip(sel_ids),
                                                    dp(d_vels), dp(true_mass), dp(vel), _lib.ip(counts),
                                                    C.cast(C.byref(ct), _lib.c_double_p), C.cast(C.byref(dt), _lib.c_double_p))
            if rc == -1 and cap < most:              # (cap too small: the error text names the size needed)
                need = re.search(r"the selections hold (\d+) rows", (c.lib.sphx_last_error(c.h) or b"").decode())
                if need:
                    cap = int(need.group(1))
                    continue
            c.check(rc)
            break
        ends = np.cumsum(sel_count)
        sels = [(d_vels[e - k_:e].copy(), sel_ids[e - k_:e].copy()) for k_, e in zip(sel_count, ends)]
        return dict(dt=dt.value, ct=ct.value, selections=sels, sel_count=sel_count, true_mass=true_mass, vel=vel,
                    counts=dict(zip(compat.SN_COUNTS, (int(v) for v in counts))))

    def sn_timing(self):
        """Device time of the selection stages of the last supernova_impulse() from HIP events, added up over its stars
        -> dict of ms: keys, bound, compact, sort, walk, kick."""
        ms = np.zeros(6)
        c = self.ctx
        c.check(c.lib.sphx_sn_last_timing(c.h, dp(ms)))
        return dict(zip(("keys", "bound", "compact", "sort", "walk", "kick"), ms.tolist()))

    # ---- the explosion and the insertion of its particles (code_running.py:361-396) on the resident state: N grows -----
    def download_rows(self, ids):
        """The rows `ids` (particle indices of the uploaded state, each once) of the state as it is on the device ->
        dict: points, velocities (n,3), mass, E_internal (n) and, with with_species=True, f_un (n,S)."""
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1))
        nr, S = ids.shape[0], self.n_species
        out = dict(points=np.empty((nr, 3)), velocities=np.empty((nr, 3)), mass=np.empty(nr), E_internal=np.empty(nr))
        fu = None
        if S > 0:
            out["f_un"] = fu = np.empty((nr, S))
        c = self.ctx
        c.check(c.lib.sphx_state_download_rows(c.h, nr, _lib.ip(ids), dp(out["points"]), dp(out["velocities"]), dp(out["mass"]),
                                               dp(out["E_internal"]), dp(fu)))
        return out

    def supernova_explosion(self, supernova_ids, d_0, t_cmb, noise_dust=None, noise_gas=None, yields=None, mu_specie=None,
                            gamma=None, star_f_un=None):
        """code_running.py:361-396 on the state as it is on the device: the rows of the stars supernova_ids come to the
        host (download_rows), compat.supernova_explosion forms the new particles from those few rows, and
        sphx_state_insert_rows (include/sphx.h) rewrites the star rows, appends the dust rows and then the gas rows, clamps
        T at t_cmb, forms mu_array and gamma_array again, and runs the search of drv:386 on the grown state.  The state
        itself stays on the device.  Afterwards self.n is N + n_dust + n_gas; download(), neighbors(),
        download_composition(), download_drag(), dust_phase(), rad_phase(), sample() and rad_transfer() work on the grown
        state at once (densities, num_densities, visc_heat and pressure are zeros until the next step); the next step()
        integrates dv = a dt for every row, as the driver does behind an insertion (drv:482-485), the one after it
        averages again.  self.first is left alone.
        -> dict: n_dust, n_gas, new_ids (the caller ids of the new rows: dust, then gas), dust_len (dust rows per star),
        explosion (compat.supernova_explosion's 16-tuple, supernova_pos being supernova_ids), info (buffers reallocated,
        rows appended, rows rewritten, rows whose T the clamp moved).
        The bits are those of compat.supernova_insert on the downloaded state.  noise_dust, noise_gas, yields: as
        compat.supernova_explosion takes them; mu_specie, gamma: the tables of drv:393-394, by default the module's.  A
        state without with_species=True needs the stars' composition rows as star_f_un (n_sn,S); mu_array and gamma_array
        of its other old rows are then left as they are.  An empty supernova_ids is a no-op (None).  Needs one step; not
        with incremental=True."""
        from . import compat
        ids = np.ascontiguousarray(np.asarray(supernova_ids, dtype=np.int64).reshape(-1))
        n_sn = ids.shape[0]
        if n_sn == 0:
            return None
        rows = self.download_rows(ids)
        fu = rows.get("f_un")
        if fu is None:
            if star_f_un is None:
                raise ValueError("a state without with_species=True needs star_f_un, the composition rows of the stars")
            fu = f64(star_f_un)
            if fu.ndim != 2 or fu.shape[0] != n_sn:
                raise ValueError("star_f_un must be (n_sn, S)")
        S = fu.shape[1]
        ex = compat.supernova_explosion(rows["mass"], rows["points"], rows["velocities"], rows["E_internal"], np.arange(n_sn), fu,
                                        d_0=d_0, noise_dust=noise_dust, noise_gas=noise_gas, yields=yields, full=True)
        (dust_comps, gas_comps, star_comps, dust_mass, gas_mass, stars_mass, newpoints, newvels, newgastype, newdusttype,
         new_eint_stars, new_eint_dust, new_eint_gas, _, dustpoints, dustvels, extra) = ex
        cat = lambda a, b: np.ascontiguousarray(np.concatenate((a, b)), dtype=np.float64)
        a_pos, a_vel = cat(dustpoints, newpoints), cat(dustvels, newvels)
        a_m, a_pt, a_E, a_f = cat(dust_mass, gas_mass), cat(newdusttype, newgastype), cat(new_eint_dust, new_eint_gas), cat(dust_comps, gas_comps)
        m_new = a_m.shape[0]
        mus, gam = compat.chem_table(S, mu_specie, "mu_specie"), compat.chem_table(S, gamma, "gamma")
        gm = se = None
        if self._with_drag:
            gm = np.ascontiguousarray(compat.grain_mass(), dtype=np.float64)
            se = np.ascontiguousarray(compat.sigma_effective(), dtype=np.float64)
            if gm.shape != (S,) or se.shape != (S,):
                raise ValueError("with_drag: grain_mass and sigma_effective hold %d species, the state %d" % (gm.shape[0], S))
        c = self.ctx
        c.check(c.lib.sphx_state_insert_rows(c.h, S, n_sn, _lib.ip(ids), dp(f64(stars_mass, (n_sn,))), dp(f64(new_eint_stars, (n_sn,))),
                                             dp(f64(star_comps, (n_sn, S))), m_new, dp(a_pos), dp(a_vel), dp(a_m), dp(a_pt), dp(a_E), dp(a_f),
                                             float(t_cmb), dp(mus), dp(gam), dp(gm), dp(se), self.k, self.dist))
        n_old = self.n
        self.n = n_old + m_new
        self._ptype = np.concatenate((self._ptype, a_pt))
        if hasattr(self, "_n_gas"):
            del self._n_gas
        self._phase_ran = True           # (mass, f_un, mu_array and gamma_array on the device are no longer the caller's)
        info = np.zeros(4, dtype=np.int64)
        c.check(c.lib.sphx_insert_last_info(c.h, _lib.ip(info)))
        return dict(n_dust=int(dust_mass.shape[0]), n_gas=int(gas_mass.shape[0]), new_ids=np.arange(n_old, n_old + m_new, dtype=np.int64),
                    dust_len=np.array(extra["dust_len"]), explosion=ex[:13] + (ids,) + ex[14:16],
                    info=dict(zip(("reallocated", "appended", "rewritten", "clamped"), (int(v) for v in info))))

    def insert_timing(self):
        """Device time of the stages of the last supernova_explosion()'s insertion from HIP events -> dict of ms: upload,
        grow, insert, search."""
        ms = np.zeros(4)
        c = self.ctx
        c.check(c.lib.sphx_insert_last_timing(c.h, dp(ms)))
        return dict(zip(("upload", "grow", "insert", "search"), ms.tolist()))

    # ---- the adaptive length scale and sizes (code_running.py:493-540) on the resident state --------------------------
    def length_scale(self, N_INT_PER_PARTICLE, raise_factor, apply=True, full=False, q=90., v_max=80000., fill=0.9):
        """code_running.py:493-540 on the state as the last step() left it (include/sphx.h sphx_state_length_scale): the
        global d from the q-th percentile of |x|^2 over the rows slower than v_max, and the new sizes - the gas rows' radii
        scaled by the change of their density since the previous applied call (1 on the first, and behind a
        supernova_explosion) and capped at d, the dust rows at d / raise_factor**(1./3.).  apply=True keeps them on the
        device: dust_phase, rad_phase, rad_transfer and supernova_impulse then read them as sizes until the next step(),
        whose search replaces them (drv:437); with forms="loop" the next step uses the new d; and d is remembered:
        dust_phase and rad_phase called with d=None use it.  apply=False changes nothing on the device.  -> dict: d,
        d_dust, max_dist, n_slow, n_nan, lo, a, b, counts (compat.SCALE_COUNTS); full=True adds sizes and
        exp_neighbor_count in the particle order of the uploaded state.  The bits are those of compat.length_scale and
        compat.adapt_sizes on download(), neighbors() and the previous call's densities.  No slow row, or a NaN d with
        apply=True: ValueError, nothing changed.  download() keeps returning the step's radii as sizes: download_sizes()
        returns the adapted ones.  Needs one step; not with incremental=True."""
        from . import compat
        n = self.n
        o = compat._scale_outputs()
        dd = np.zeros(1); counts = np.zeros(len(compat.SCALE_COUNTS), dtype=np.int64)
        sizes = rev = None
        if full:
            sizes, rev = np.zeros(n), np.zeros(n, dtype=np.int64)
        c = self.ctx
        c.check(c.lib.sphx_state_length_scale(c.h, float(v_max) ** 2, float(np.true_divide(q, 100)), float(N_INT_PER_PARTICLE), float(fill),
                                              float(raise_factor), 1 if apply else 0, _lib.ip(o[0]), _lib.ip(o[1]), _lib.ip(o[2]), dp(o[3]),
                                              dp(o[4]), dp(o[5]), dp(o[6]), dp(dd), _lib.ip(counts), dp(sizes), _lib.ip(rev)))
        out = compat._scale_result(*o)
        out["d_dust"] = float(dd[0])
        out["counts"] = dict(zip(compat.SCALE_COUNTS, (int(v) for v in counts)))
        if full:
            out["sizes"], out["exp_neighbor_count"] = sizes, rev
        if apply:
            self._scale_d = out["d"]
        return out

    def download_sizes(self):
        """The adapted sizes of the last length_scale(apply=True) -> (N,) in the particle order of the uploaded state.
        Raises once a step() has replaced them, or when none were formed."""
        out = np.empty(self.n)
        c = self.ctx
        c.check(c.lib.sphx_state_download_sizes(c.h, dp(out)))
        return out

    def scale_timing(self):
        """Device time of the last length_scale() from HIP events -> dict of ms: keys, select, reverse_counts, adapt,
        write_back."""
        from . import compat
        ms = np.zeros(5)
        c = self.ctx
        c.check(c.lib.sphx_scale_last_timing(c.h, dp(ms)))
        return dict(zip(compat.SCALE_STAGES, ms.tolist()))

    # ---- the census, the ordered selections and the stellar clock (code_running.py:244, 339-342, 604, 616-622, 636, 656-664) ----
    def set_star_ages(self, star_ages):
        """The driver's star_ages (N,) in the particle order of the uploaded state, kept on the device by particle id
        (include/sphx.h sphx_state_set_star_ages).  supernova_explosion extends them by -2 for every new row (drv:371)."""
        c = self.ctx
        c.check(c.lib.sphx_state_set_star_ages(c.h, dp(f64(star_ages, (self.n,)))))
        self._has_ages = True

    def download_star_ages(self):
        """-> star_ages (N,) as they are on the device.  Raises before they are set."""
        out = np.empty(self.n)
        c = self.ctx
        c.check(c.lib.sphx_state_download_star_ages(c.h, dp(out)))
        return out

    def advance_star_ages(self, dt):
        """drv:604 on the device: star_ages[(particle_type == 1) & (star_ages > -2)] += dt.  Raises before they are set."""
        c = self.ctx
        c.check(c.lib.sphx_state_advance_star_ages(c.h, float(dt)))

    def last_dt(self):
        """The last step's dt (what download()["dt"] holds), with nothing downloaded."""
        dt = C.c_double(0.0)
        c = self.ctx
        none = [None] * 9
        c.check(c.lib.sphx_state_download(c.h, *none, C.cast(C.byref(dt), _lib.c_double_p)))
        return dt.value

    def census(self, mu_specie=None):
        """The sums, counts and the maximum the driver reports every pass (drv:341, 465-468, 616-617, 636, 656-658) from the
        state as it is on the device (include/sphx.h sphx_state_census) -> compat.census's dict: gas_mass, star_mass,
        dust_mass, nondust_mass, total_mass, the counts, max_star_mass, star_massfrac, star_numfrac, net_accel, momentum,
        kinetic, internal and, with with_species=True, gas_, star_ and dust_mass_by_species (else None).  58 numbers come
        back, no array.  The bits are those of compat.census on download() and download_composition(), whatever order the
        state is stored in.  The state is only read."""
        from . import compat
        S = self.n_species
        mus = compat.chem_table(S, mu_specie, "mu_specie") if S else None
        tot = np.zeros(compat.CENSUS_FIXED + 3 * S); counts = np.zeros(4, dtype=np.int64); mx = np.zeros(1)
        c = self.ctx
        c.check(c.lib.sphx_state_census(c.h, dp(mus), dp(tot), _lib.ip(counts), dp(mx)))
        return compat._census_result(tot, counts, mx[0], S)

    def census_timing(self):
        """Device time of the last census() from HIP events -> dict of ms: prepare (the id -> slot map), chunk_sums, totals,
        read_back."""
        from . import compat
        ms = np.zeros(4)
        c = self.ctx
        c.check(c.lib.sphx_census_last_timing(c.h, dp(ms)))
        return dict(zip(compat.CENSUS_STAGES, ms.tolist()))

    # ---- the picture of the cloud (code_running.py:563-597): the state projected onto a pixel grid ----
    def project(self, half_width, npix, d=None, axes=(1, 2), center=(0, 0), depth=None, fields=None, stars=False):
        """The state as it is on the device integrated along a coordinate axis onto a pixel grid (include/sphx.h
        sphx_state_project; after the first step) -> compat.project_maps' dict: (n_v, n_u) arrays gas_column, dust_column,
        gas_temperature, dust_temperature, count (those of `fields`; None: all), skipped and pairs.  Only the images come
        back, no N-sized array.  d: the driver's global d (drv:68); None: the d remembered from the last
        length_scale(apply=True).  axes = (a_u, a_v), the line of sight is the third coordinate; center, half_width and
        npix: a pair (u, v) or one value for both; depth = (lo, hi) keeps the particles with lo <= line-of-sight
        coordinate < hi.  Sizes are the step's radii (download()["sizes"]), as sample() reads them.  The driver's own
        window (drv:563-597) is axes=(1, 2), center=0, half_width=sqrt(length_scale()["max_dist"] * 11 / 9).
        stars=True adds star_ids, star_uv (n, 2) and star_mass of the stars inside the window (and the depth), in
        ascending particle id.  The bits are those of compat.project_maps on download(), whatever order the state is
        stored in.  The step loop is not disturbed."""
        from . import compat
        d = self._d_or_remembered(d)
        flds = compat.MAP_FIELDS if fields is None else tuple(fields)
        *geom, out = compat._map_args(axes, center, half_width, npix, depth, flds)
        c = self.ctx
        rc, res = compat._map_call(c.lib.sphx_state_project, (c.h, float(d)), geom, out)
        c.check(rc)
        if stars:
            ax, ce, hw, _, dep = geom
            sel = self._select(1)
            rows = self.download_rows(sel["ids"]) if sel["ids"].shape[0] else dict(points=np.zeros((0, 3)))
            p = rows["points"]
            au, av = int(ax[0]), int(ax[1])
            keep = (np.abs(p[:, au] - ce[0]) <= hw[0]) & (np.abs(p[:, av] - ce[1]) <= hw[1])
            if dep is not None:
                w = p[:, 3 - au - av]
                keep &= (w >= dep[0]) & (w < dep[1])
            res["star_ids"] = sel["ids"][keep]
            res["star_uv"] = np.ascontiguousarray(p[keep][:, [au, av]])
            res["star_mass"] = sel["mass"][keep]
        return res

    def map_timing(self):
        """Device time of the last project() from HIP events -> dict of ms: footprints (with the id -> slot map),
        count_scan (with the host's wait for the pair count), list_build, tiles, read_back."""
        from . import compat
        ms = np.zeros(5)
        c = self.ctx
        c.check(c.lib.sphx_map_last_timing(c.h, dp(ms)))
        return dict(zip(compat.MAP_STAGES, ms.tolist()))

    # ---- what the run's self-gravity does to its energy (include/sphx.h sphx_state_gravity_potential) ----
    def gravity_potential(self, by_id=False):
        """Potential energy of the state as it is on the device, in the mode of the step's gravity (gravity="direct", or
        "tree" with the step's kernels, ws and order - over a side grid built for the call as compat.grav_potential_tree
        builds it, not over the step's own cells; raises when the simulation has no gravity) -> dict: U = 1/2 sum m phi [J] in the
        order of the ordered totals over the particle ids (the same bits in every storage order), eps (the softening:
        median of the sizes, 0 before the first step), total_mass, bad (rows whose phi is not finite) and, with by_id,
        phi (n,) [J/kg] - the bits of compat.grav_potential_direct / _tree on download() and download_composition()'s
        mass.  Four numbers come back unless by_id.  The state and what the next step reads are left as they were."""
        phi = np.empty(self.n) if by_id else None
        out = np.zeros(4)
        c = self.ctx
        c.check(c.lib.sphx_state_gravity_potential(c.h, dp(phi), dp(out)))
        res = dict(U=float(out[0]), total_mass=float(out[1]), eps=float(out[2]), bad=int(out[3]))
        if by_id:
            res["phi"] = phi
        return res

    def gravpot_timing(self):
        """Device time of the last gravity_potential() from HIP events -> dict of ms (compat.GRAVPOT_STAGES)."""
        from . import compat
        ms = np.zeros(4)
        c = self.ctx
        c.check(c.lib.sphx_gravpot_last_timing(c.h, dp(ms)))
        return dict(zip(compat.GRAVPOT_STAGES, ms.tolist()))

    def energy(self):
        """The energy budget of a self-gravitating run -> dict: kinetic and internal as census() forms them (its bits; the
        sums by species are left out, so no mu_specie table is needed), potential from gravity_potential(), total (their
        sum) and virial = 2 kinetic / |potential|.  No N-sized array is downloaded."""
        from . import compat
        tot = np.zeros(compat.CENSUS_FIXED); counts = np.zeros(4, dtype=np.int64); mx = np.zeros(1)
        c = self.ctx
        c.check(c.lib.sphx_state_census(c.h, None, dp(tot), _lib.ip(counts), dp(mx)))      # (no sums by species: no table needed)
        cen = compat._census_result(tot, counts, mx[0], 0)
        pot = self.gravity_potential()
        kin, inte, U = float(cen["kinetic"]), float(cen["internal"]), pot["U"]
        with np.errstate(all="ignore"):
            virial = float(np.float64(2.0 * kin) / np.float64(abs(U)))
        return dict(kinetic=kin, internal=inte, potential=U, total=kin + inte + U, virial=virial)

    def _select(self, ptype, ages=False, f_un=False, window=None):
        """The rows of a type in ascending particle id from the device (include/sphx.h sphx_state_census_select)."""
        from . import compat
        S = self.n_species if f_un else 0
        cap = int(np.count_nonzero(self._ptype == ptype))
        o = compat._select_outputs(cap, S)
        lo, hi = (0., 0.) if window is None else window
        c = self.ctx
        c.check(c.lib.sphx_state_census_select(c.h, int(ptype), 0 if window is None else 1, float(compat.solar_mass), float(lo),
                                               float(hi), cap, _lib.ip(o[0]), _lib.ip(o[1]), dp(o[2]), dp(o[3]),
                                               dp(o[4]) if ages else None, dp(o[5])))
        return compat._select_result(o)

    def dust_temperatures(self):
        """drv:620: T[particle_type == 2] in the particle order of the uploaded state, compacted on the device."""
        return self._select(2)["T"]

    def supernova_schedule(self):
        """drv:244, 339-342 -> compat.supernova_schedule's dict (supernova_pos, max_rel_age, max_star_mass, n_star): the
        device compacts the star rows (id, mass, age), the host evaluates the reference's expression on them.  Raises
        before star_ages are set."""
        from . import compat
        return compat._schedule_of(self._select(1, ages=True))

    def run_outputs(self, OVERALL_AGE, mu_specie=None):
        """The entries of the driver's closing np.savez (drv:670) that depend on the state -> compat.run_outputs' dict, from
        census() and the AGB rows (drv:660-664) compacted on the device.  Needs with_species=True and star_ages."""
        from . import compat
        S = self.n_species
        if S < 1:
            raise RuntimeError("the simulation carries no composition (with_species=True and a state with f_un)")
        mus = compat.chem_table(S, mu_specie, "mu_specie")
        cen = self.census(mus)
        out = {nm: cen[nm] for nm in ("gas_mass_by_species", "star_mass_by_species", "dust_mass_by_species")}
        rows = self._select(1, ages=True, f_un=True, window=compat.AGB_WINDOW)
        out.update(compat._agb_outputs(self.n, rows, OVERALL_AGE, mus))
        return out

    # ---- snapshot / restart and per-step diagnostics (the reference only wrote summary
    # statistics at the end of a run, sph/code_running.py:670, and printed the mass-weighted net
    # accelerations every step, sph/code_running.py:465-468) ----------------------------------------
    def snapshot(self, path, state):
        """Write a restartable particle-state snapshot (.npz): the downloaded dynamic arrays plus the
        static per-particle arrays of `state` (mass, particle_type, mu_array, gamma_array, f_un).  Once a dust_phase has
        run, mass, mu_array, gamma_array and f_un are no longer static: they then come from download_composition()."""
        d = self.download()
        out = dict(points=d["points"], velocities=d["velocities"], total_accel=d["total_accel"],
                   E_internal=d["E_internal"], T=d["T"], sizes=d["sizes"], dt=np.float64(d["dt"]),
                   first=np.int64(1 if self.first else 0), n_neigh=np.int64(self.k), dist=np.float64(self.dist))
        for key in ("mass", "particle_type", "mu_array", "gamma_array"):
            out[key] = np.asarray(state[key], dtype=np.float64)
        if state.get("f_un") is not None:
            out["f_un"] = np.asarray(state["f_un"], dtype=np.float64)
        if self._phase_ran:
            out.update(self.download_composition())
        if self._ptype.shape[0] != out["particle_type"].shape[0]:      # (a supernova_explosion has appended rows since)
            out["particle_type"] = self._ptype.copy()
        if self._has_ages:
            out["star_ages"] = self.download_star_ages()
        np.savez(path, **out)

    @classmethod
    def from_snapshot(cls, path, device=None, **kw):
        z = dict(np.load(path, allow_pickle=False))
        state = {k_: z[k_] for k_ in ("points", "velocities", "total_accel", "E_internal", "T", "mass",
                                       "particle_type", "mu_array", "gamma_array")}
        state["f_un"] = z.get("f_un")
        if "star_ages" in z and "star_ages" not in kw:
            kw["star_ages"] = z["star_ages"]
        sim = cls(state, n_neigh=int(z["n_neigh"]), dist=float(z["dist"]), device=device, **kw)
        sim.first = bool(int(z["first"]))
        return sim, state

    def diagnostics(self, state):
        """Mass-weighted net acceleration, momentum and energies of the current state
        (sph/code_running.py:465-468 prints the first of these every step).  It downloads the whole state: census()
        forms the same quantities on the device, in a fixed order of summation."""
        d = self.download()
        # (once a dust_phase has run the caller's masses are stale: the device's)
        m = self.download_composition()["mass"] if self._phase_ran else np.asarray(state["mass"], dtype=np.float64)
        mt = m.sum()
        return dict(net_accel=(d["total_accel"] * m[:, None]).sum(axis=0) / mt,
                    momentum=(d["velocities"] * m[:, None]).sum(axis=0),
                    kinetic=0.5 * float((m * (d["velocities"] ** 2).sum(axis=1)).sum()),
                    internal=float(d["E_internal"].sum()), dt=d["dt"])

    def stats(self):
        return self.ctx.stats()

    def reset_stats(self):
        self.ctx.reset_stats()
        self._failures_seen = None
