/* sphx.h - C ABI of libsphx.so: the MI355X (gfx950) implementation of the SPH inner
 * loop of dmuley/sph-code.
 *
 * The reference has no FFI; its boundary for this path is the set of module-level
 * Python callables of sph/navier_stokes_cleaned.py ("nsc") that the driver
 * sph/code_running.py ("drv") invokes as nsc.<name>(...).  Each entry point below
 * names the reference callable it replaces (file:line).  The Python side
 * (sph_code_amd/compat.py) binds them with ctypes and keeps the reference's
 * positional signatures and return tuples.
 *
 * Conventions
 *   - plain pointers and sizes only; every array is C-contiguous; "f64" = double.
 *   - host-pointer entry points copy in, run on the context's HIP stream, copy out
 *     and synchronise before returning; no pointer is retained after return.
 *   - *_dev entry points take DEVICE pointers (memory owned by the caller, e.g. a
 *     torch tensor's data_ptr()) and are asynchronous on the context's stream.
 *   - return value: 0 = ok, < 0 = error (SPHX_E_*); sphx_last_error(ctx) gives text.
 *   - one context per GPU per process; a context is not thread-safe; different
 *     contexts may be used concurrently.
 *   - missing neighbours are encoded as index == n (reference convention, nsc:545-548)
 *     and contribute zero to every sum (the reference raises IndexError).
 */
#ifndef SPHX_H
#define SPHX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPHX_OK            0
#define SPHX_E_ARG        -1   /* bad argument (null pointer, k > 64, n < 1 ...) */
#define SPHX_E_HIP        -2   /* a HIP runtime call failed                      */
#define SPHX_E_NOMEM      -3   /* device allocation failed                       */
#define SPHX_E_STATE      -4   /* call sequence error (e.g. step before upload)  */

#define SPHX_MAX_K        64   /* one neighbour per lane of a 64-wide wavefront  */
#define SPHX_MAX_SPECIES  32

typedef struct sphx_ctx sphx_ctx;

/* Physical constants read by the path (nsc:21-52).  Defaults are the values the
 * golden fixtures were generated with; sphx_set_constants overrides them. */
typedef struct sphx_constants {
    double k_B;      /* nsc:22  scipy.constants.Boltzmann                  */
    double amu;      /* nsc:25  atomic mass constant                       */
    double m_h;      /* nsc:29  1.0008 amu                                 */
    double m_0;      /* nsc:36  10^1.5 solar masses                        */
    double dt_0;     /* nsc:38  250000 yr                                  */
    double max_age;  /* drv:79  3e7 yr                                     */
    double pos_clamp;/* drv:233 1e11 AU                                    */
    double solar_luminosity; /* nsc:31 3.846e26 W                          */
    double c;        /* nsc:27  scipy.constants.c                          */
} sphx_constants;

/* Per-pass timing / traffic model of the last sphx_step call. */
typedef struct sphx_stats {
    double ms_grid;        /* bbox + cell hash + counting sort + state permute */
    double ms_search;      /* kNN kernel                                        */
    double ms_prep;        /* gather-record build                               */
    double ms_density;     /* pass 1: rho, rho_dust, n, grad P                  */
    double ms_pi;          /* pass 2: Pi_i + crossing time (0 in pairwise steps)  */
    double ms_visc;        /* pass 3: viscous accel + heat (pairwise steps: the fused pass, crossing time included) */
    double ms_integrate;   /* dt + leapfrog                                     */
    double ms_total;       /* events around the whole step                      */
    int64_t n;             /* particles                                         */
    int64_t steps;         /* steps accumulated in the ms_* sums                */
    int64_t candidates;    /* candidate distance evaluations in the search      */
    int64_t retries;       /* searches repeated with a larger radius            */
    int64_t cells;         /* cells of the last grid                            */
    int64_t refresh_steps; /* steps whose kNN came from the Verlet lists         */
    int64_t rebuild_steps; /* steps with cell sort + full search                 */
    double  cell_size;     /* edge of the last grid's cells                     */
    double  ms_gravity;    /* self-gravity (0 unless sphx_state_set_gravity)    */
    int64_t fallback_queries; /* last step (or sphx_dev_search): queries the grouped search left to the general kernel */
    double  ms_species;    /* species pass of the step (+ metallicity, AGB yields); ms_density excludes it */
    int64_t short_rows;    /* searches that gave up after the last radius of the retry ladder with fewer than K
                              neighbours although more particles exist (pathological states only; 0 otherwise) */
    int64_t detail_steps;  /* steps accumulated in ms_prep .. ms_integrate, ms_gravity, ms_species (sphx_set_timing_detail) */
    int64_t far_queries;   /* last hinted search but one: queries outside the grid box with a search sphere wider than 8 cells */
    int64_t outlier_levels;/* last hinted search: nested outlier levels it was given (0: none built) */
    /* Failure counters (particles, summed over the steps since sphx_reset_stats; 0 in a sane run).  The reference guards
     * its loop with nan_to_num alone (sph/code_running.py:233-238, 460-463, 490-491) and carries on; so does the step -
     * these say how often that guard was needed.  Counted on the device by ballot where the values are in registers.  */
    int64_t bad_accel;     /* pressure / viscous / drag acceleration NaN or inf before nan_to_num (rho_i = 0 or NaN, ...)   */
    int64_t bad_energy;    /* E or heat x dt NaN or inf before the nan_to_num of drv:490                                    */
    int64_t bad_state;     /* updated position or velocity NaN or inf (the next step's clamp, drv:233-238, catches them)    */
    int64_t bad_h;         /* kNN radius 0 (coincident points), NaN or inf                                                  */
    int64_t search_steps;  /* steps accumulated in ms_search                                                                */
    /* The last hinted search's tie list (near ties of two consecutive ranks, which the grouped search leaves to the tie
     * blocks of the list-mode launch): read when sphx_get_stats is called, behind the stream.                         */
    int64_t tie_entries;   /* entries that search reserved; may exceed tie_capacity (the queries that did not fit went to
                              the general kernel).  0 if it kept no tie list                                           */
    int64_t tie_capacity;  /* entries its tie list had room for (npad / 16 + 1024)                                    */
    /* Sums the LDS passes did not have to finish because they were NaN already (counted since sphx_reset_stats or the
     * last state upload; read when sphx_get_stats is called, behind the stream).                                      */
    int64_t visc_blobs_settled; /* pass 3: blobs of 128 rows whose own m Pi is NaN in every row: neither staged nor walked */
    int64_t pi_waves_settled;   /* pass 2: waves (16 rows of one blob) that went on with the crossing-time term alone
                                   after every row's sum had become NaN                                                */
    int64_t visc_launches_skipped; /* pass 3 (fused single-GPU step, LDS passes): launches that returned at once because pass 2
                                      had marked no blob for them - it writes the NaN rows itself and marks the blobs with
                                      other rows; the blobs pass 3 does not walk count in visc_blobs_settled           */
    int64_t update_split_steps; /* steps (since sphx_reset_stats) whose leapfrog/energy update split its rows in two classes
                                   by a byte that pass 2 left: rows whose viscous sums are settled (NaN) - neither stored
                                   by a pass nor loaded by the update - and the rows pass 3 sums (fused single-GPU step,
                                   LDS passes, neither drag nor gravity); counted on the host                          */
} sphx_stats;

/* ---- context ----------------------------------------------------------------------- */
int         sphx_create(sphx_ctx** out, int device);
void        sphx_destroy(sphx_ctx* ctx);
const char* sphx_last_error(const sphx_ctx* ctx);
int         sphx_version(void);
/* How the library was built ("gfx950 experiments=0": it holds no timing experiments or diagnostics that add launches
 * or change results), and the SPHX_* environment variables a context read when it was created ("NAME=value ...":
 * performance tunables only, read once, in sphx_create).  A benchmark line carries both, so that it can be shown to be
 * the configuration the parity tests ran.                                                                         */
const char* sphx_build_info(void);
const char* sphx_tunables(const sphx_ctx* ctx);
/* Hardware self-test of the search's matrix-core cull (sphx_knn_group.hip, phase A): `blocks` random 32 x 32 blocks of
 * candidates and queries with coordinates in [-E, E] (cell units, E <= 40) through v_mfma_f32_32x32x16_f16 exactly as the
 * search forms them, compared with fp64.  max_err_over_E2: the largest |D - (d^2 - R^2 (1 + pad))| / E^2 met; kappa: the
 * bound the search's certification assumes; wrong_signs: entries beyond that bound whose sign differed (must be 0).
 * Test infrastructure (tests/test_gpu_parity.py); replaces nothing in the reference. */
/* Self-test of the grid build's single-launch prefix sum (sphx_grid.hip: lookback_scan_kernel) against rocPRIM's scan on
 * the device: n pseudo-random counts through both, entries that differ in *mismatches (must be 0); *single_launch: whether
 * n ran through the single-launch form (scans of more than 512 tiles of 8192 items take rocPRIM's either way).
 * Test infrastructure; replaces nothing in the reference. */
int sphx_selftest_scan(sphx_ctx* ctx, int n, unsigned seed, long long* mismatches, int* single_launch);
/* Self-test of the fused step's cell and blob order (sphx_grid.hip).  On the caller's n positions (host arrays) and a grid
 * of cells of `cell_size`, the cells are counted, scanned and scattered once; the order is then finished twice - by the
 * per-cell pass (member sort, curve counts, host cues), scan and scatter, and by the fused step's kernels (curve counts from
 * the scatter, scan, member order by counting in the gather, the cues kernel) - and the finished cell order, the blob
 * order, the curve's starts and total and the two cues are compared on the device: entries that differ in *mismatches
 * (must be 0).  *new_chain_taken: 1 when the fused step's kernels ran (0: the curve's code space was refused for this
 * grid, nothing to compare).  Test infrastructure; replaces nothing in the reference. */
int sphx_selftest_grid_order(sphx_ctx* ctx, int n, const double* x, const double* y, const double* z, double cell_size,
                             long long* mismatches, int* new_chain_taken);
int sphx_selftest_mfma_cull(sphx_ctx* ctx, double E, int blocks, unsigned seed, double* max_err_over_E2,
                            double* wrong_signs, double* kappa);
/* Page-locked host memory for the big arrays the array entry points hand back ((N,K) int64 + float64 from
 * sphx_neighbors: 640 MB at N = 1e6, K = 40): device-to-host copies into it run at the link's rate instead of
 * being staged through the runtime's bounce buffers (~4x).  Any host pointer is accepted everywhere; this is
 * an optimisation a binding may use for its output arrays.  SPHX_E_NOMEM if the pages cannot be locked.   */
int         sphx_host_alloc(void** out, size_t bytes);
int         sphx_host_free(void* p);
int         sphx_set_constants(sphx_ctx* ctx, const sphx_constants* c);
int         sphx_get_constants(const sphx_ctx* ctx, sphx_constants* c);
/* Search tuning (performance only, never results): the step loop searches inside
 * rscale * h_previous (default 1.2) and bins particles into cells of edge
 * cell_factor * mean(h) (default 0.6).  Values <= 0 keep the current setting. */
int         sphx_set_tuning(sphx_ctx* ctx, double rscale, double cell_factor);
/* sphx_step times the whole call (ms_total) and every step's search launches (ms_search) with HIP events always; one event
 * per pass (ms_grid, ms_prep ... ms_integrate, ms_gravity, ms_species; stats.detail_steps counts the steps they cover) only
 * when asked: an event record between two dependent kernels costs the stream ~10 us.  Off by default (SPHX_TIMING_DETAIL=1). */
int         sphx_set_timing_detail(sphx_ctx* ctx, int on);
/* Incremental search (off by default).  With verlet != 0 a full search also keeps each
 * particle's 64 nearest candidates; following steps take the exact kNN from those lists as long
 * as it can be PROVEN exact from the displacements since (sphx_refresh.hip), else the step
 * rebuilds.  It pays when the fastest particle moves much less than 0.08 h per step; in the
 * BASELINE workloads (dt >= dt_0/5, sph/code_running.py:226) it does not, hence the default.
 * rscale_build (default 1.3, <= 0 keeps) is the search radius factor on rebuilding steps.      */
int         sphx_set_incremental(sphx_ctx* ctx, int verlet, double rscale_build);

/* ---- nsc.neighbors(points, dist, N_NEIGH)                          nsc:541-552 ----- *
 * Exact k nearest neighbours (Euclidean) within `dist`; `eps` is accepted for API
 * compatibility (the reference passes 0.1 to cKDTree) and ignored: the result is the
 * eps = 0 answer, which satisfies every guarantee of the eps > 0 one.
 *   points  (n,3) f64      idx      (n,k) int64, sorted by distance, column 0 = self,
 *                                   missing = n
 *   dist_out (n,k) f64 (missing = 0)   nontriv (n,) int64   h (n,) f64 = max distance  */
int sphx_neighbors(sphx_ctx* ctx, int64_t n, int k, const double* points, double dist,
                   double eps, int64_t* idx, double* dist_out, int64_t* nontriv, double* h);

/* ---- nsc.hydro_update(neighbor, points, mass, sizes, f_un, particle_type, T, mu_array,
 *                       gamma_array, velocities)                     nsc:556-671 ----- *
 * visc_mode 0 = "ref_axis0": Pi_i = sum_k pi_ik, the axis repair of nsc:649.
 * visc_mode 1 = "pairwise": the per-pair pi_ik stays inside the force sum (the Monaghan form of the
 *   loop version, nsc:802-808).  With dx, dv relative to neighbor[i,0], g_j = [type_j == 0], gb / ga
 *   the kernel gradients of nsc:591 (clipped under sphx_set_clip_grad) / nsc:592, alpha = 1:
 *     w_ik   = min(0, (dv . dx) / sqrt(r^2 + 0.01 h_j^2))                     nsc:643-644
 *     rho_ab = (rho_j + rho_i) / 2,  c_ab = (c_j + c_i) / 2                   nsc:646-647
 *     pi_ik  = -(alpha/2) (2 c_ab - 3 w_ik) w_ik / rho_ab                     nsc:649 term
 *     B_ik   = 1/2 pi_ik [m_j g_j gb + m_i g_i ga]
 *     visc_accel_i = -sum_k B_ik,  visc_heat_i = (m_i/2) sum_k B_ik . dv     nsc:651-654
 *   gb, ga are non-negative multiples of -dx and pi_ik > 0 only where dv . dx < 0, so visc_heat >= 0 for
 *   every particle.  Passes: density, then ONE viscous pass that forms pi_ik per pair and casts the
 *   crossing-time vote (the Pi_i pass is not run).  The other outputs are those of mode 0, bit for bit.
 *   Any other visc_mode: SPHX_E_ARG.  The argument alone decides (sphx_set_visc_mode plays no part).
 * Outputs keep the reference's sign (+grad P / rho) and layouts:
 *   hydro_accel, visc_accel (n,3); visc_heat, rho, nden, rho_dust (n,); f_un_nb (s,n).
 * Any output pointer may be NULL (that output is skipped).
 * neighbor (here and in the loop forms below) may be NULL = "the (n,k) list of the previous array call
 * on this context": the reference's loop passes one list to eight functions (drv:451-458), which is
 * 320 MB of PCIe traffic each at N = 1e6, K = 40.  SPHX_E_STATE if no list of that shape is held
 * (a search or a step on the context discards it).                                      */
int sphx_hydro_update(sphx_ctx* ctx, int64_t n, int k, int s, const int64_t* neighbor,
                      const double* points, const double* mass, const double* sizes,
                      const double* f_un, const double* particle_type, const double* T,
                      const double* mu_array, const double* gamma_array,
                      const double* velocities, int visc_mode,
                      double* hydro_accel, double* visc_accel, double* visc_heat,
                      double* rho, double* nden, double* f_un_nb, double* rho_dust);

/* ---- loop forms (h = (m/m_0)^(1/3) d, d = the driver-injected global nsc.d) ---------- */
/* nsc.density(points,mass,particle_type,neighbor)                    nsc:693-702        */
int sphx_density(sphx_ctx* ctx, int64_t n, int k, const double* points, const double* mass,
                 const double* particle_type, const int64_t* neighbor, double d, double* out);
/* nsc.dust_density(points,mass,neighbor,particle_type,sizes)         nsc:704-717        */
int sphx_dust_density(sphx_ctx* ctx, int64_t n, int k, const double* points, const double* mass,
                      const int64_t* neighbor, const double* particle_type, const double* sizes,
                      double* out);
/* nsc.num_dens(mass,points,mu_array,neighbor)                        nsc:744-753        */
int sphx_num_dens(sphx_ctx* ctx, int64_t n, int k, const double* mass, const double* points,
                  const double* mu_array, const int64_t* neighbor, double d, double* out);
/* nsc.del_pressure(points,mass,particle_type,neighbor,E_internal,gamma_array) nsc:755-774 */
int sphx_del_pressure(sphx_ctx* ctx, int64_t n, int k, const double* points, const double* mass,
                      const double* particle_type, const int64_t* neighbor,
                      const double* E_internal, const double* gamma_array, double d,
                      double* out /* (n,3) */);
/* nsc.artificial_viscosity(neighbor,points,particle_type,sizes,mass,densities,velocities,
 *                          T,gamma_array,mu_array)                   nsc:788-816        */
int sphx_artificial_viscosity(sphx_ctx* ctx, int64_t n, int k, const int64_t* neighbor,
                              const double* points, const double* particle_type,
                              const double* sizes, const double* mass, const double* densities,
                              const double* velocities, const double* T,
                              const double* gamma_array, const double* mu_array, double d,
                              double* visc_accel /* (n,3) */, double* visc_heat /* (n,) */);
/* nsc.crossing_time(neighbor,velocities,sizes,particle_type)         nsc:776-786        */
int sphx_crossing_time(sphx_ctx* ctx, int64_t n, int k, const int64_t* neighbor,
                       const double* velocities, const double* sizes,
                       const double* particle_type, double* out /* scalar */);
/* nsc.net_impulse(points,mass,sizes,velocities,particle_type,neighbor,f_un) nsc:719-742
 * mean_grain_mass/mean_cross are the per-particle sums meff.f_un, seff.f_un (nsc:720-726),
 * formed by the caller from nsc.grain_mass / nsc.sigma_effective.                        */
int sphx_net_impulse(sphx_ctx* ctx, int64_t n, int k, const double* points, const double* mass,
                     const double* sizes, const double* velocities, const double* particle_type,
                     const int64_t* neighbor, const double* mean_grain_mass,
                     const double* mean_cross, double* accel_onto /* (n,3) */,
                     double* accel_reaction /* (n,3) */);

/* Softened direct-sum gravity on host arrays: accel (n,3).  sizes != NULL: eps = median(sizes)
 * (nsc:358, as grav_force_calculation_new(mass, points, sizes) takes it), else eps = softening.   */
int sphx_gravity_direct(sphx_ctx* ctx, int64_t n, const double* mass, const double* points,
                        const double* sizes, double softening, double G, double* accel);

/* The same sum by multipoles of a cell pyramid over a search-style grid (cells sized for k_cells
 * neighbours, 40 if < 1): level-l cells of 2^l fine cells a side carry (mass, centre of mass) and, at
 * order 2 (sphx_set_gravity_order; the default), their second moments; a particle sums the cells that
 * are children of its parent's +-ws neighbours but not its own +-ws neighbours, level by level, and
 * the particles of the +-ws level-1 cells directly.  ws = 1..4.  rms force error against the exact sum:
 * order 2: ~0.1 % at ws = 1, ~0.01 % at ws = 2; order 1: ~1 %, ~0.2 %.  Every cell is softened like a
 * particle (nsc:385): the expansion is that of the softened kernel.                                 */
int sphx_gravity_tree(sphx_ctx* ctx, int64_t n, const double* mass, const double* points,
                      const double* sizes, double softening, double G, int ws, int k_cells,
                      double* accel);

/* The gravitational potential beside the two sums above: the same walks, records and softening, one scalar per target.
 *   per row     phi_i = -G sum_{j != i} m_j / sqrt(|x_j - x_i|^2 + eps^2)   [J/kg], eps taken exactly as the acceleration
 *               calls take it (sizes != NULL: median(sizes) on the device, else softening)
 *   self term   row i is left out of its own sum BY INDEX: it is never added and then taken off again
 *   coincident  a different row at the same position contributes -G m_j / eps; with eps = 0 and r = 0 nothing, as in the
 *               acceleration sum
 *   total       U = 1/2 sum_i m_i phi_i   (sphx_state_gravity_potential)
 *   tree cell   a cell carries M at c and, at order 2, S_ab about c.  With r = c - x and s^2 = r^2 + eps^2 its term is the
 *               second-order expansion of the same softened kernel,
 *                   phi_cell = -G [ M / s + 3/2 (r.S.r) / s^5 - 1/2 tr S / s^3 ]
 *               whose negative gradient in x is the acceleration term of sphx_gravity_tree (7.5, 1.5, 3).  Order 1 keeps
 *               M / s.  The trace term stays: the softened kernel is not harmonic.
 * pot (n).  accel (n,3) is nullable; where given it holds the bits of sphx_gravity_direct / sphx_gravity_tree.
 * sphx_gravity_tree_pot uses the grid (k_cells = 40), pyramid and eps of sphx_gravity_tree, and sphx_set_gravity_order. */
int sphx_gravity_direct_pot(sphx_ctx* ctx, int64_t n, const double* mass, const double* points,
                            const double* sizes, double softening, double G, double* accel, double* pot);
int sphx_gravity_tree_pot(sphx_ctx* ctx, int64_t n, const double* mass, const double* points,
                          const double* sizes, double softening, double G, int ws, double* accel, double* pot);
/* Device time of the stages of the last potential call on this context (HIP events), ms: [0] inputs onto the device and
 * eps, [1] grid and pyramid (tree; the direct sum: 0), [2] the sum and the totals, [3] outputs onto the host.         */
int sphx_gravpot_last_timing(sphx_ctx* ctx, double ms[4]);

/* The same sum over a cloud held in nparts parts (part_of[i] in 0 .. nparts-1; a part may be empty): the out-of-core /
 * multi-domain form, and the computation a decomposed run does across ranks, on one context.  Each part builds the grid
 * and pyramid over its OWN particles and sums its own field as sphx_gravity_tree does (nparts = 1 gives that call's bits).
 * To every other part q it exports its mass as a flat list decided against Q_q, the bounding box of q's particles: a
 * cell c travels as one multipole record {M, centre; second moments} iff it is the first cell on the way down from the
 * top whose box stands at least ws of its longest edges clear of Q_q (face cells reach out to the part's true bounding
 * box: the grid clamps outliers into them); the particles of level-1 cells never so accepted travel as {x, y, z, m}.
 * Every massive particle is in exactly one record, and every multipole has the clearance of the single-domain
 * interaction list.  Each part then ADDS the field of the lists it received (fp64, in list order: sources in part
 * order, cells top-down in index order, then particles in cell order - the same bits on every run).  Cell centres
 * travel relative to the centre of the global bounding box.  ws = 0..4; ws = 0 exports everything as particles and sums
 * the own field directly: the exact sum of sphx_gravity_direct.  counts (nparts, nparts, 2), nullable: cells and
 * particles part a sent to part b.  The export holds one flag per (peer, cell): nparts x cells must stay below 2^31.  */
int sphx_gravity_tree_parts(sphx_ctx* ctx, int64_t n, const double* mass, const double* points,
                            const double* sizes, double softening, double G, int ws, int k_cells, int nparts,
                            const int32_t* part_of, double* accel, int64_t* counts);

/* AGB dust and gas return per star: calculate_interpolation, sph/config_helper.py:180-211, on the
 * splines of interpolate_amounts (config_helper.py:138-178; RectBivariateSpline kx = ky = 1).
 * Spline o has ntx[o] / nty[o] knots and (ntx[o]-2)*(nty[o]-2) coefficients; tx, ty, coeffs are the
 * splines' arrays one after the other (SciPy's get_knots() / get_coeffs()).  x = metallicity,
 * y = mass; arguments outside the knot range are clamped as FITPACK does.  dust[i, mapto[o]] =
 * spline_o (a repeated target keeps the last spline), then / divisor and clipped at 0.
 * gas_out (and composition, both (n, nspecies)) may be NULL.  nspecies 6..32, nspl <= 32.        */
int sphx_agb_yields(sphx_ctx* ctx, int64_t n, const double* masses, const double* metallicities,
                    int nspl, const int32_t* ntx, const int32_t* nty, const double* tx,
                    const double* ty, const double* coeffs, const int32_t* mapto, double divisor,
                    int nspecies, const double* mu_specie, const double* composition,
                    double solar_mass, double* dust_out /* (n,nspecies) */,
                    double* gas_out /* (n,nspecies) */);

/* ---- the driver's inline integrator statements as array functions ----------------------- *
 * The reference has no function for these: they are straight-line statements inside its time
 * loop.  Each entry replaces the cited block on host arrays; the device code is the one the fused
 * step loop runs (sphx_leapfrog.h).  Pinned by tests/golden/driver_integrator.npz.          */
/* code_running.py:223-229: dt[i] from crossing time ct[i] (nsc.crossing_time's return value) and
 * first[i] (age == 0): dt_0/10 | max(dt_0/5, min(2 dt_0, ct)); ct > MAX_AGE -> MAX_AGE/100.   */
int sphx_dt_rule(sphx_ctx* ctx, int64_t n, const double* ct, const int32_t* first, double* dt);
/* code_running.py:233-238: |x| <= 1e11 AU, nan_to_num on points and velocities ((n,3), in place) */
int sphx_clamp_arrays(sphx_ctx* ctx, int64_t n, double* points, double* velocities);
/* code_running.py:460-491: pressure_accel = delp/rho [gas]; visc = drag_on_gas rho_dust/rho [gas] +
 * drag_reaction + av_accel (drag pointers NULL: av_accel alone); limiter (:475); total = grav +
 * pressure + visc (grav NULL: none); points += total dt^2/2 + v dt; v += (total + old)/2 dt
 * (old_accel NULL: shapes differ, dv = total dt, :484-485); E += av_heat dt; T = E mu m_h/(gamma m k).
 * In place: points, velocities (n,3), E_internal (n,); out: total_accel (n,3), T (n,).        */
int sphx_leapfrog(sphx_ctx* ctx, int64_t n, double* points, double* velocities, double* total_accel,
                  const double* old_accel, double* E_internal, double* T, const double* mass,
                  const double* mu, const double* gamma, const double* ptype, const double* grav_accel,
                  const double* delp, const double* densities, const double* dust_densities,
                  const double* drag_on_gas, const double* drag_reaction, const double* av_accel,
                  const double* av_heat, double dt);

/* ---- device-resident simulation state: the fused hot path of drv:217-491 ------------- *
 * upload once, step many times (search -> dt -> sums -> leapfrog, nothing leaves HBM),
 * download when needed.  Particle order on the device changes every step (cell sort);
 * download returns arrays in the original order (by particle id).
 *   pos, vel, accel_old (n,3); mass, ptype, T, mu, gamma, E (n,); f_un (n,s) or NULL.   */
int sphx_state_upload(sphx_ctx* ctx, int64_t n, int s, const double* pos, const double* vel,
                      const double* mass, const double* ptype, const double* f_un,
                      const double* T, const double* mu, const double* gamma,
                      const double* E_internal, const double* accel_old);
/* Enable the dust->gas drag of nsc.net_impulse (nsc:719-742) inside the step loop:
 * visc_accel = drag*rho_dust/rho*[gas] + reaction + viscous accel (drv:455,462-463,473).
 * mean_grain_mass / mean_cross (n,) as in sphx_net_impulse; NULL disables.  Call directly after
 * sphx_state_upload.  The reaction (nsc:741) is an ordered scatter: contributions added by source particle (caller
 * index), then list position - np.add.at's order, the same bits on every run (n*K*32 B of device memory). */
int sphx_state_set_drag(sphx_ctx* ctx, const double* mean_grain_mass, const double* mean_cross);
/* Species pass inside the step: when sphx_state_upload was given f_un, every sphx_step (hydro_update mode) also forms
 * F[s,i] = sum_k m_j/(mu_j amu) [gas_j] f_un[j,s] W (nsc:624-627) on its own neighbour list.  With an AGB table set
 * (config_helper.py:138-178: nspl degree-1 splines over (metallicity, mass) as sphx_agb_yields takes them; nspl = 0
 * switches it off) the same pass leaves, without another trip over memory, the per-particle metallicity
 * Z_i = sum_{s>=6} F[s,i] mu_s / sum_s F[s,i] mu_s (the expression of code_running.py:663 on the smoothed composition)
 * and the AGB dust yields of config_helper.py:183-189 at (Z_i, m_i) - BASELINE configs[4].
 * sphx_state_download_species: F (s,n) species-major as nsc:671 returns it, Z (n,), agb_dust (n,s); caller order;
 * any pointer may be NULL.                                                                                          */
int sphx_state_set_agb(sphx_ctx* ctx, int nspl, const int32_t* ntx, const int32_t* nty, const double* tx,
                       const double* ty, const double* coeffs, const int32_t* mapto, double divisor,
                       const double* mu_specie, double solar_mass);
int sphx_state_download_species(sphx_ctx* ctx, double* F, double* Z, double* agb_dust);
/* Step mode "loop forms": on != 0 makes sphx_step evaluate, on its own neighbour list, exactly what the
 * reference's time loop evaluates (drv:451-458): density, dust_density, num_dens, del_pressure,
 * artificial_viscosity and crossing_time in their loop forms (nsc:673-816; smoothing length
 * h(m) = (m/m_0)^(1/3) d with the driver's global d, clipped gradients, physical sign), then
 * pressure_accel = delp / rho [gas], visc_accel = av[0] (+ drag), limiter, leapfrog, E += av[1] dt
 * (drv:460-491).  The default (on == 0) uses the vectorised sums of nsc.hydro_update instead.
 * Call after sphx_state_upload; `dist` of sphx_step is the search bound the driver passes (drv:437). */
int sphx_state_set_loop_forms(sphx_ctx* ctx, int on, double d);
/* Physics option, off by default.  hydro_update's neighbour-side kernel gradient
 * -6 C h_j^-9 (h_j^2 - r^2)^2 is not clipped for r > h_j (nsc:591) - reproduced for parity, but it grows as
 * r^4 and makes long runs of the vectorised form diverge; the reference's own time loop uses the loop forms,
 * which clip it (nsc:689).  on != 0 clips it (0 for h_j^2 - r^2 <= 0) in sphx_hydro_update, sphx_step and
 * the sphx_dev_* passes of this context.                                                          */
int sphx_set_clip_grad(sphx_ctx* ctx, int on);
/* Viscosity of sphx_step (hydro_update mode) and of the sphx_dev_* passes of this context: 0 = "ref_axis0" (the default),
 * 1 = "pairwise" (the formula at sphx_hydro_update).  Pairwise steps run density, then one fused viscous pass (no Pi_i
 * pass: stats.ms_pi stays 0, ms_visc covers the fused pass).  SPHX_E_ARG for any other mode, and for mode 1 in loop-form
 * mode (sphx_state_set_loop_forms), whose viscosity is pairwise already; sphx_state_set_loop_forms(on) likewise refuses
 * a context in mode 1.  Kept across sphx_state_upload.                                                                  */
int sphx_set_visc_mode(sphx_ctx* ctx, int mode);
/* Self-gravity inside the step loop (drv:448-449,477): mode 1 = direct summation with Plummer
 * softening eps = median(h) of the step (nsc:358), G m_j (x_j - x_i) / (|x_j - x_i|^2 + eps^2)^(3/2)
 * summed over ALL particles - the sum the reference's tree approximates (sphx_gravity_direct).
 * O(N^2): meant for N up to a few 10^5.  mode 2 = the same sum by cell-pyramid multipoles
 * (sphx_gravity_tree with ws = 1, order 2; SPHX_GRAV_WS / sphx_set_gravity_order override), ~1.5e3 terms
 * per particle.  mode 0 switches it off.  Call after sphx_state_upload. */
int sphx_state_set_gravity(sphx_ctx* ctx, int mode, double G);
/* Multipole order of the tree's cells (sphx_gravity_tree and mode 2 above): 1 = monopoles, 2 (default) =
 * monopoles + second moments about each cell's centre of mass, the second-order Taylor term of the
 * softened kernel - ws = 1 then beats the accuracy monopoles need ws = 2 for, at 40 % of the cost
 * (DESIGN 5.7).                                                                                         */
int sphx_set_gravity_order(sphx_ctx* ctx, int order);
/* Potential and potential energy of the resident state at its current positions and masses (the ones
 * sphx_state_download and the composition download return), in the mode of sphx_state_set_gravity (SPHX_E_STATE when
 * none is set): the state is gathered into particle-id order on the device and handed to the routine behind
 * sphx_gravity_direct_pot / sphx_gravity_tree_pot (ws and order of the step; eps = median of the state's sizes, 0 before
 * the first step), so phi by id is that call's bits on the downloaded state.  pot_by_id (n), nullable.
 * out[0] = U = 1/2 sum_i m_i phi_i, summed over the particle ids in the order of the library's ordered totals (chunks of
 * 256 ids left to right, lane l of 256 adds chunks l, l + 256, ..., then a binary tree): the same bits on every call and
 * in every storage order, no floating-point atomic.  out[1] = sum m (same order), out[2] = eps, out[3] = the number of
 * rows whose phi is not finite.  Tree mode builds a grid and pyramid of its own for the current positions and leaves
 * everything the next step reads as it was.  Only the potential: no acceleration is written.                          */
int sphx_state_gravity_potential(sphx_ctx* ctx, double* pot_by_id, double out[4]);
/* One or more passes of the hot path.  k = N_NEIGH, dist = distance_upper_bound of
 * nsc:544 (<= 0 or inf: unbounded), first != 0: the first step uses dt_0/10 (drv:223-224);
 * fixed_dt > 0 overrides the crossing-time rule (drv:225-229).                           */
int sphx_step(sphx_ctx* ctx, int nsteps, int k, double dist, int first, double fixed_dt);
/* Any output pointer may be NULL.  The particle state (pos ... sizes) belongs to the loop alone; rho, nden
 * and visc_heat are the last step's pass outputs, which live in work buffers the array entry points above
 * also use - ask for them before calling those on the same context (or give the loop a context of its own). */
int sphx_state_download(sphx_ctx* ctx, double* pos, double* vel, double* accel,
                        double* E_internal, double* T, double* sizes, double* rho,
                        double* nden, double* visc_heat, double* dt_last);
/* P_i = n_i k_B T_i (n,), caller order: number density (nsc:607) and temperature of ONE instant - the one the last step's
 * sums were formed at.  (The reference's own `pressure` line is commented out, nsc:608; north_star names P as an output.
 * T of sphx_state_download is the UPDATED temperature, drv:491; the one the sums read is kept by the update at no cost.)
 * Zeros before the first step.  Same caveat as rho / nden above about array calls on the same context.            */
int sphx_state_download_pressure(sphx_ctx* ctx, double* pressure);
/* ---- fields at arbitrary points: nsc.neighbors_arb, density_arb, dust_density_arb, temperature_arb,
 *      dust_temperature_arb, photoionization_arb                                nsc:1422-1527 ----- *
 * With C = 315/(64 pi), h(m) = (m/m_0)^(1/3) d, r = |x_k - x_0| for query point x_0 and particle k:
 *   Wg_k = m_k C h(m_k)^-9 (h(m_k)^2 - r^2)^3 (nsc:673-676),  Wd_k = the same with s_k = sizes[k] (nsc:678-681),
 *   g_k = [type_k == 0], u_k = [type_k == 2]; neither weight is clipped, the "> 0" masks below do that.
 * Over the members k of the point's ball (nsc:1422-1426), and 0 from every function when the ball has at most one
 * member (nsc:1432):
 *   density          sum of the positive Wg g                                            nsc:1428-1443
 *   dust_density     sum of the positive Wd u                                            nsc:1445-1461
 *   temperature      nan_to_num(sum a / sum b) over a = Wg g T > 0, b = Wg g             nsc:1463-1486
 *   dust_temperature nan_to_num(sum Wd u T / sum Wd u) over Wd u > 0                     nsc:1488-1508
 *   photoionization  sum w nan_to_num(value) / sum w over w = (1 - r^2/h^2)^3 g n_part > 0; 0/0 stays NaN  nsc:1510-1527
 * sphx_arb_fields (nsc:1422-1527), grid form: the ball is the EXACT set |x_k - x_0| <= radius (the reference asks
 * cKDTree for eps = 0.1, whose answer depends on the tree's traversal); radius <= 0: max(sizes).  points (n,3), mass,
 * particle_type (n,); sizes, T, n_part, value (n,) may be NULL, which skips the outputs that need them (value = the
 * reference's `photoionization` argument).  arb_points (m,3); a point with a NaN or inf coordinate gets count 0 and zeros.
 * Outputs (m,), any may be NULL.  count: the ball's members; NULL: only min(count, 2) is formed.  *candidates: pair
 * evaluations performed.  The same inputs give the same bits on every call, in whatever order the points are given.
 * m = 0 writes nothing.  SPHX_E_ARG: m < 0, n < 1, a NULL required pointer, radius <= 0 without sizes.
 * ball_id != 0 names the ball: the caller promises that every call with this id on this context is given the same points
 * and arb_points.  The context keeps the last ball's geometry on the device - the particles' cell list and sorted
 * positions, the query points and their sorted order - and a call that names it again neither uploads points and
 * arb_points nor rebuilds any of that: only mass ... value go up and the records and sums are formed (the reference's
 * five functions are called one after the other on one list, nsc:1428-1527).  Without any field output (count alone)
 * no record and no sum is formed at all.  ball_id = 0: nothing is kept.  One ball is held at a time; sphx_arb_fields_list
 * drops it, sphx_state_sample replaces it with an unnamed one.
 * One reading differs from the list form: temperature and photoionization also demand a positive weight of their
 * terms.  With T_k < 0 (n_part_k < 0) the reference's masks pass particles OUTSIDE their own support, anywhere in the
 * ball; the grid form's cost follows the supports, so it leaves them out.  Nothing changes for T >= 0, n_part >= 0. */
int sphx_arb_fields(sphx_ctx* ctx, int64_t n, const double* points, const double* mass,
                    const double* particle_type, const double* sizes, const double* T, const double* n_part,
                    const double* value, double d, int64_t m, const double* arb_points, double radius,
                    double* density, double* dust_density, double* temperature, double* dust_temperature,
                    double* photoionization, int64_t* count, int64_t* candidates, int64_t ball_id);
/* sphx_arb_fields_list (nsc:1428-1527), list form: the balls are given, as CSR - row_start (m+1) int64, non-decreasing
 * (else SPHX_E_ARG), members int64 particle ids; an id < 0 or >= n is skipped.  Each row is summed in list order, every
 * listed particle counts (no radius), count = the row's length.  This honours a list made elsewhere exactly - the
 * reference's own eps = 0.1 lists included.                                                                         */
int sphx_arb_fields_list(sphx_ctx* ctx, int64_t n, const double* points, const double* mass,
                         const double* particle_type, const double* sizes, const double* T, const double* n_part,
                         const double* value, double d, int64_t m, const double* arb_points,
                         const int64_t* row_start, const int64_t* members, double* density, double* dust_density,
                         double* temperature, double* dust_temperature, double* photoionization, int64_t* count,
                         int64_t* candidates);
/* sphx_state_sample (nsc:1422-1527): sphx_arb_fields' grid form on the step loop's device-resident state - the positions,
 * masses, types, T and sizes sphx_state_download would return at this moment; n_part, value (n,) in the caller's
 * particle order, or NULL.  SPHX_E_STATE before the first sphx_step (sizes do not exist yet).  The loop is not disturbed:
 * the next sphx_step gives the bits it would have given without this call.  Its work buffers are shared with the array
 * entry points: the caveat at sphx_state_download (rho, nden, visc_heat) applies.                                    */
int sphx_state_sample(sphx_ctx* ctx, double d, const double* n_part, const double* value, int64_t m,
                      const double* arb_points, double radius, double* density, double* dust_density,
                      double* temperature, double* dust_temperature, double* photoionization, int64_t* count,
                      int64_t* candidates);
/* Device time of the last of the three calls above on this context, from HIP events on its stream, in ms:
 * ms[0] inputs going up, ms[1] reductions, grid build, query sort, records (host waits between them included),
 * ms[2] the sum and gate kernels (list form: the row kernel), ms[3] outputs coming back.  Measurement aid for
 * nsc:1422-1527's replacement; replaces nothing in the reference.                                                   */
int sphx_arb_last_timing(sphx_ctx* ctx, double ms[4]);
/* ---- radiative transfer: the geometry and the deposition of nsc.rad_heating              nsc:922-965 ----- *
 * rad_heating's star selection and luminosities (nsc:897-921) and its composition chemistry (nsc:967-1017) stay with the
 * caller; these entry points take the selected sources a_s (n_src,3) with their `luminosities`, the sampled targets b_q
 * (n_dst,3), and return what nsc:922-965 form.  With C2 = 3 pi / 80 (the reference's W6_constant, nsc:48 - not the
 * 315/(64 pi) of the sums), particles p of EVERY type at x_p with h_p = sizes, m_p, mu_p, sigma_p = cross_array:
 *   w_p = C2 h_p^-2 sigma_p m_p / (mu_p amu)                                                       nsc:928
 *   ray (s,q), u = b_q - a_s:  d2_p = |(x_p - a_s) x u|^2 / |u|^2                                  nsc:927
 *   blocked[s,q] = sum_p [d2_p < h_p^2] w_p,   star_distance[s,q] = |u|                            nsc:928-931
 *     - the whole infinite line, matter behind the star included, as the reference has it.
 *   over the particles g with ptypes != 1, in the caller's order (G of them):
 *   gd[q,g] = |x_g - b_q|,  sd2[s,g] = |x_g - a_s|                                                 nsc:941-944
 *   lum_factor[s,g] = nan_to_num(sd2 sum_q((gd + 1.)^-2 / star_distance[s,q] blocked[s,q]) / sum_q (gd + 1.)^-2)
 *     - the 1. is one metre, as written in the reference                                           nsc:949
 *   extinction[g] = w_g,  a_int = pi h_g^2,  df[s,g] = (nan_to_num(sd2)^2 + min(sizes over ptypes == 0)^2) 4 pi
 *   l[s,g] = nan_to_num(exp(-nan_to_num(lum_factor)) / df L_s a_int extinction)                    nsc:954-961
 *   lf2[g] = sum_s l dt solar_luminosity,   momentum[g] = sum_s (x_g - a_s)/sd2 l / m_g dt / c     nsc:963-965
 * nan_to_num is NumPy's; everything else plain IEEE: a degenerate ray (a_s == b_q) has column 0 and distance 0, and its
 * 0/0 zeroes lum_factor[s,:]; n_dst = 0 gives lum_factor = 0; n_src = 0 gives lf2 = momentum = 0.  The kernel compares
 * |(x_p - a) x u|^2 with h_p^2 |u|^2 instead of dividing: the column is a top-hat, and a pair within rounding of its
 * edge may fall on either side (of either evaluation).  The sums over p run in chunks of the particle range fixed by
 * (n, n_src n_dst) alone and are added in chunk order, without atomics: the same inputs give the same bits on every
 * call.  solar_luminosity, c, amu: sphx_constants.
 * mode SPHX_RAD_LINE: the above.  SPHX_RAD_SEGMENT, an extension the reference does not have (parity unpinned, like
 * clip_grad and visc_mode 1): only particles whose foot point lies between source and target block the ray,
 * 0 <= (x_p - a).u < |u|^2, half-open - a particle AT the source counts, one AT the target does not; lum_factor and
 * everything after it use the column the mode produced.
 * SPHX_E_ARG: a negative count, a NULL required pointer, an unknown mode.
 * Layout constants a test of the kernels' seams reads: the column kernel stages SPHX_RAD_TILE particles at a time, a
 * workgroup holds SPHX_RAD_WG_RAYS rays, the particle range is split into up to ceil(2048 / ray tiles) chunks of whole
 * tiles; the deposit kernel takes SPHX_RAD_SRC_CHUNK sources at a time.                                              */
#define SPHX_RAD_LINE        0
#define SPHX_RAD_SEGMENT     1
#define SPHX_RAD_TILE        256
#define SPHX_RAD_WG_RAYS     256
#define SPHX_RAD_SRC_CHUNK   16
/* sphx_rad_columns (nsc:922-931): the columns alone - the optical depth between any two point sets.  points (n,3);
 * sizes, mass, mu, cross (n,); blocked (n_src,n_dst); star_distance (n_src,n_dst) or NULL.  n = 0 gives zero columns;
 * n_src n_dst = 0 writes nothing and returns 0.                                                                    */
int sphx_rad_columns(sphx_ctx* ctx, int64_t n, const double* points, const double* sizes, const double* mass,
                     const double* mu, const double* cross, int64_t n_src, const double* src, int64_t n_dst,
                     const double* dst, int mode, double* blocked /* (n_src,n_dst) */, double* star_distance /* may be NULL */);
/* sphx_rad_transfer (nsc:922-965): all of the above.  ptypes (n,) f64 0/1/2; luminosities (n_src,).  Outputs in the
 * reference's order over the G non-star particles - lf2 (G,), momentum (G,3), extinction (G,) - then blocked,
 * star_distance (n_src,n_dst) and lum_factor (n_src,G); any may be NULL.  SPHX_E_ARG when no particle has ptypes == 0
 * (the reference raises on the empty min of nsc:957), n = 0 included.                                              */
int sphx_rad_transfer(sphx_ctx* ctx, int64_t n, const double* points, const double* ptypes, const double* mass,
                      const double* sizes, const double* cross, const double* mu, int64_t n_src, const double* src,
                      const double* luminosities, int64_t n_dst, const double* dst, double dt, int mode, double* lf2,
                      double* momentum, double* extinction, double* blocked, double* star_distance, double* lum_factor);
/* sphx_state_rad_transfer (nsc:922-965): sphx_rad_transfer on the step loop's device-resident state - the positions,
 * masses, types, mu and sizes sphx_state_download would return at this moment; cross (n,) in the caller's particle order
 * (as sphx_state_sample takes n_part).  The sums run in the caller's order: the bits are those of sphx_rad_transfer on
 * the downloaded state.  SPHX_E_STATE before the first sphx_step (sizes do not exist yet).  It works in buffers of its
 * own: the next sphx_step gives the bits it would have given without this call.                                    */
int sphx_state_rad_transfer(sphx_ctx* ctx, const double* cross, int64_t n_src, const double* src,
                            const double* luminosities, int64_t n_dst, const double* dst, double dt, int mode, double* lf2,
                            double* momentum, double* extinction, double* blocked, double* star_distance,
                            double* lum_factor);
/* Device time of the last of the three calls above on this context, from HIP events on its stream, in ms: ms[0] inputs
 * going up and prepared (w_p, h_p^2, the non-star list, min(sizes); one host wait), ms[1] the column kernel and the sum
 * of its chunks, ms[2] spread and deposit, ms[3] outputs coming back.  Measurement aid for nsc:922-965's replacement;
 * replaces nothing in the reference.                                                                               */
int sphx_rad_last_timing(sphx_ctx* ctx, double ms[4]);
/* ---- nsc.rad_cooling(positions, particle_type, masses, sizes, cross_array, f_un, neighbor, mu_array, T, dt)
 *                                                                                         nsc:1019-1176 ----- *
 * Recombination and its cooling on the list `neighbors` returned (drv:276).  sizes and cross_array are accepted by the
 * reference and never read: they are not arguments here.  Species columns of f_un (n,s), s >= 6: 0 H2, 1 He, 2 H, 3 H+,
 * 4 He+, 5 e-.  With W(p,j) = Weigh2(x_p, x_j, m_p, d) (nsc:673-676, h(m) = (m/m_0)^(1/3) d), g_p = [type_p == 0],
 * t4 = T_p / 1e4, for every gas row j with a gas neighbour and every p = neighbor[j,k]:
 *   base = W / (mu_p m_h) g_p (m_h, not amu);  n_e, n_H+, n_He+, n_H0 = base f_p[5], f_p[3], f_p[4], f_p[2], each kept
 *   where > 0;  rel_w = W g [W g > 0] / Weigh2(x_p, x_p, m_p, d)                           nsc:1044-1057
 *   H_eff = 4.13e-19 t4^(-0.7131 - 0.0115 ln t4), He_eff = 2.72e-19 t4^-0.789, H2_eff = 7.3e-23 0.5 (T_p/100)^(1/2),
 *   e_H = (0.684 - 0.0416 ln t4 + 0.54 t4^0.37) k T_p, e_He = (0.684 - 0.0416 ln(t4/4)) k T_p       nsc:1060-1067
 *   over the entries with n_e > 0: num_e = sum n_e, A = sum H_eff n_e, B = sum He_eff n_e; num_H+ = sum n_H+,
 *   num_He+ = sum n_He+; Cn = sum H2_eff n_H0 over n_H0 > 0                                 nsc:1075-1084
 *   f_e = min((A num_H+ + B num_He+) / num_e dt, 0.9999), s_H = nan_to_num(A/(A+B)), s_He = nan_to_num(B/(A+B)),
 *   f_H = f_e s_H, f_He = f_e s_He, f_Hn = min(Cn dt, 0.9999),
 *   E_H = sum H_eff n_e e_H s_H dt, E_He = sum He_eff n_e e_He s_He dt (n_e > 0)             nsc:1088-1097
 *   into every neighbour p: energy[3] += E_H rel_w, energy[4] += E_He rel_w, rec[2] += f_Hn [n_H0 > 0] rel_w,
 *   rec[3], rec[4], rec[5] += f_H, f_He, f_e [n_e > 0] rel_w, rel += rel_w                   nsc:1102-1110
 * then per particle (nsc:1112-1176): rec, energy /= rel + 1e-90; H+_frac, He+_frac, e_frac = f[5] rec[3,4,5];
 * mult_factor; f[1] += He+_frac mult, f[2] += H+_frac mult, f[3,4,5] -= ...; rec[2] capped at 0.9999,
 * f[0] += f[2] rec[2] / 2, f[2] -= f[2] rec[2]; energy = energy[3] f[3] + energy[4] f[4] (f before the transfers);
 * every particle's s species - stars and dust included - divided by their sum.  f is nan_to_num(f_un) throughout.
 * Quirks of the reference kept on purpose:
 *   1. np.maximum(a, b, c) at nsc:1122 has three positional arguments and the third is `out`:
 *      mult_factor = max(H+ ratio, He+ ratio); the electron ratio never enters.
 *   2. nsc:1124-1125 test mf2 > 0.9999 and mf2 < 0.9999: mf2 == 0.9999 exactly keeps its value.
 *   3. nan_to_num maps +-inf to +-DBL_MAX, not to 0; the x/0 ratios of nsc:1122 rely on it.
 *   4. The two mass-budget prints (nsc:1027, 1172) are not reproduced.
 *   5. Only rows 2-5 of rec_array and rows 3-4 of the energy accumulator are ever non-zero.
 *   A row with num_e = 0 is NaN inside and contributes exactly zero through nan_to_num and the pair masks.
 * Two repairs: np.min(x, 0.9999) at nsc:1089 and nsc:1094 passes 0.9999 as `axis` and raises
 * TypeError; the reading implemented - and pinned by tests/golden/cool_*.npz - is np.minimum.
 * Ours: a list entry outside [0, n) (the missing-neighbour value n) contributes nothing; the coefficients of a neighbour
 * whose T is not in (0, inf) are zero.  A row is taken to hold distinct indices, as `neighbors` returns them; a repeated
 * index is added once per occurrence (the reference's fancy-indexed += adds it once).
 * The sums over K run in list order; a particle adds the rows that hold it in ascending row index, the order of the
 * reference's loop, from a reverse list (4 bytes per pair) sorted per particle: no floating-point atomic, the same inputs
 * give the same bits on every call.  m_0, m_h, k_B: sphx_constants.
 * Outputs: final_comp (n,s), energy (n,), rec_array (s,n); row_table (n,6) or NULL: per row f_Hn, f_H, f_He, f_e (each
 * nan_to_num'ed, as the scatter reads them), E_H, E_He; zeros for a row that does not contribute.
 * SPHX_E_ARG: a NULL required pointer, n < 1, k < 1, s < 6, non-finite dt or d, n k beyond 2^31.
 * SPHX_COOL_WG: lanes (rows, particles) of a workgroup of its kernels - a layout constant the tests' sizes straddle. */
#define SPHX_COOL_WG         256
int sphx_rad_cooling(sphx_ctx* ctx, int64_t n, int k, int s, const double* points, const double* ptype,
                     const double* mass, const double* f_un, const int64_t* neighbor, const double* mu, const double* T,
                     double dt, double d, double* final_comp, double* energy, double* rec_array,
                     double* row_table /* may be NULL: (n,6) */);
/* Device time of the last sphx_rad_cooling call on this context, from HIP events on its stream, in ms: ms[0] inputs going
 * up, records and the K-major list, ms[1] the row pass, ms[2] reverse list (scan, one host wait, fill, sort), gather and
 * epilogue, ms[3] outputs coming back.  Measurement aid; replaces nothing in the reference.                          */
int sphx_cool_last_timing(sphx_ctx* ctx, double ms[4]);
/* ---- nsc.supernova_destruction(points, velocities, neighbor, mass, f_un, mu_array, sizes, densities, particle_type)
 *                                                                                         nsc:1211-1263 ----- *
 * Shock sputtering of dust on the list `neighbors` returned (drv:411).  For a gas row j (type_j == 0) and every entry
 * i = neighbor[j,k] that is dust (type_i == 2), with s = sizes, r^2 = |x_i - x_j|^2, C_i = [m_i > crit_mass]:
 *   wd = m_i 315 (s_i^2 - r^2)^3 / (64 pi s_i^9) (Weigh2_dust, nsc:678-681), w0 = the same at r^2 = 0
 *   rho = wd [wd > 0] C_i;  the row contributes only if sum_k rho > 0                      nsc:1237-1239
 *   v = |v_i - v_j| / 1000                                                                 nsc:1241-1242
 *   eff_c(v), eff_si(v): linear interpolation on the 8 knots (knots_v; knots_c, knots_si: nsc:148-150); 0 outside
 *   [knots_v[0], knots_v[7]], the last knot itself inside; species t takes none, eff_c or eff_si by species_curve[t]
 *   ff_t = (dens_j C_i / critical_density) (eff_t nan_to_num(rho / w0));  ff_t >= 0.99 -> 0.99   nsc:1242-1245
 *   lost_t = ff_t f_un[i,t] N_i,  N_i = m_i / (mu_i amu)                                   nsc:1247-1251
 *   in ascending j, list order inside a row:  accept = (acc[i,t] + lost_t < limit_i);  lost_t *= accept;
 *   acc[i,t] += lost_t;  reup[j,t] += lost_t                                               nsc:1252-1258
 *   frac_destruction = nan_to_num(acc / N), frac_reuptake = nan_to_num(reup / N) (N_j of row j itself)  nsc:1260-1261
 * Repair: the reference's tuple of interpolants has 14 entries for 15 species and raises on its
 * first contributing row; the selector is an argument of length s here.  The reference's tuple is
 * (0,0,0,0,0,0,1,2,1,2,1,1,1,0), padded with 0 ("none") up to s: none of the entries it wrote changes (index 6, e-,
 * keeps the carbon curve as committed; a dust row has f[6] = 0).
 * Quirks of the reference kept on purpose:
 *   1. guard_mode SPHX_DUST_GUARD_COUNT: limit_i = 1 - the comparison of a count of atoms (~1e50) with 1.
 *   2. NaN x False = NaN: a NaN lost_t is not accepted and still poisons acc[i,t] and reup[j,t], as in NumPy.
 *   3. A negative f_un entry gives a negative lost_t, which is always accepted.
 *   4. The d argument of Weigh2_dust is unused: it is no argument here.
 * Ours: guard_mode SPHX_DUST_GUARD_FRACTION sets limit_i = N_i - a species' accumulated loss stays below the
 * particle's count of atoms, which is what the comparison evidently meant; the reference cannot produce it (pinned by
 * tests/dust_oracle.py alone).  A list entry outside [0, n) contributes nothing.  Only (gas row, dust entry) pairs are
 * formed and a species whose selector is 0 loses exactly 0: the reference's 0 x inf = NaN of a non-dust entry or an
 * unselected species with non-finite data does not arise.  A row is taken to hold distinct indices; a repeated index
 * counts once per occurrence, in list order (the reference's fancy-indexed += adds it once).
 * Each dust particle walks the rows that hold it in ascending (j, k) from a reverse list (4 bytes per pair, key
 * j k_total + k) sorted per particle, and leaves one 32-bit word of accept bits per pair; each row then sums its K pairs
 * in list order under those bits.  No floating-point atomic: the same inputs give the same bits on every call.
 * knots_v must be finite and strictly increasing.  amu: sphx_constants.
 * Outputs: frac_destruction, frac_reuptake (n,s); counts int64[5] or NULL, over the (pair, selected species) elements
 * of contributing rows: lost > 0 before the guard; of those accepted; of those rejected; of the rejected those with
 * lost < limit on their own (rejected by what was accumulated); elements capped at 0.99.
 * SPHX_E_ARG: a NULL required pointer, n < 1, k < 1 or k > 64, s < 1 or s > SPHX_MAX_SPECIES, a non-finite crit_mass,
 * critical_density or knot, knots_v not increasing, a selector outside 0..2, an unknown guard mode, n k beyond 2^31.
 * SPHX_DUST_WG: lanes (particles, rows) of a workgroup of its kernels.                                              */
#define SPHX_DUST_WG              256
#define SPHX_DUST_GUARD_COUNT     0
#define SPHX_DUST_GUARD_FRACTION  1
int sphx_supernova_destruction(sphx_ctx* ctx, int64_t n, int k, int s, const double* points, const double* velocities,
                               const int64_t* neighbor, const double* mass, const double* f_un, const double* mu,
                               const double* sizes, const double* densities, const double* ptype, double crit_mass,
                               double critical_density, const int32_t* species_curve /* int32[s]: 0 none, 1 c, 2 si */,
                               const double knots_v[8], const double knots_c[8], const double knots_si[8], int guard_mode,
                               double* frac_destruction, double* frac_reuptake, int64_t* counts /* int64[5] or NULL */);
/* Device time of the last sphx_supernova_destruction call on this context, from HIP events on its stream, in ms: ms[0]
 * inputs going up, records and the K-major list, ms[1] the reverse list (scan, one host wait, fill, sort), ms[2] the dust
 * pass, ms[3] the row pass and the outputs coming back.  Measurement aid; replaces nothing in the reference.        */
int sphx_dust_last_timing(sphx_ctx* ctx, double ms[4]);
/* ---- nsc.supernova_impulse(points, masses, supernova_pos, ptypes)                               nsc:1192-1204 ----- *
 * The kick of an exploding star on the gas around it, for n_sn stars in the order given - the driver's loop drv:350-352.
 * The module globals are arguments: mass_displaced (nsc:1193: 194.28 solar_mass) and kick_energy = supernova_energy 0.736
 * (nsc:1200; 2 kick_energy is exact, so it is the reference's 2 supernova_energy 0.736).  For each star ku:
 *   s_i = (dx^2 + dy^2) + dz^2, dx = points[i] - points[ku] per column                      nsc:1194 (NumPy's order)
 *   the candidates: the rows with ptypes == 0, by s ascending                               nsc:1195-1196
 *   selected while running < mass_displaced, running the LEFT-TO-RIGHT sum of their masses  nsc:1197 (np.cumsum)
 *   true_mass = the sum of the selected masses                                              nsc:1198
 *   vel = sqrt(2 kick_energy / true_mass)                                                   nsc:1200
 *   d_vels = (dx / sqrt(s)) vel per component, s formed again as above                      nsc:1201
 *   velocities_inout[selected] += d_vels                                                    drv:351-352
 * Star t + 1's additions land on top of star t's, as the driver's sequential += does; positions and masses do not
 * change between the stars.  The selection and kick of a star are written behind the previous star's in sel_ids, d_vels.
 * Ours, where the reference leaves it open or differs:
 *   1. Ties: rows at bit-equal distance are ordered by ASCENDING INDEX (the stable order).  The reference's np.argsort is
 *      the default quicksort, not stable: its order among exact ties is unspecified, ours is one of those it may give.
 *   2. A NaN distance orders last, by index.
 *   3. true_mass is summed in the library's fixed order (sphx_ordered_totals) over the selection IN SORTED ORDER: chunks
 *      of 256 consecutive rows summed left to right, lane l of 256 adds the chunks l, l + 256, ... in order, the lanes by
 *      a binary tree (l += l + 128, l + 64, ...).  np.sum's pairwise order differs: at most (n_sel - 1) 2^-53 relative.
 *   4. Masses that are not all positive and finite: the reference's mask cumsum < M need not be a prefix then; ours is
 *      the prefix up to the first row whose running sum is not < mass_displaced (a NaN mass ends it).  Such rows are
 *      counted among the candidates (bad_mass; once per pass over them: again when a star is done again).
 * Quirks kept: a gas row at distance 0 (a gas "star", a coincident row) gets NaN kicks - 0 / 0 - and is counted
 * (zero_distance), not guarded; an empty selection gives true_mass = 0 and vel = inf.
 * The same inputs give the same bits and the same counts on every call: the key bound comes from integer histograms,
 * the candidates are sorted by (distance bits, index), no floating-point atomic is used.
 * Outputs: sel_count int64[n_sn]; sel_ids int64[cap], d_vels (cap,3): the first sum(sel_count) rows are written;
 * true_mass, vel [n_sn]; velocities_inout (n,3) or NULL; counts int64[SPHX_SN_NCOUNT] or NULL, over the call:
 * candidates sorted, sorts in one workgroup's LDS (up to SPHX_SN_LDS_CAP candidates), sorts in global memory,
 * widenings (a walk ran out of candidates and the star was redone over every gas row), selected rows at distance 0,
 * candidates whose mass is not positive and finite.
 * SPHX_E_ARG: a NULL required pointer, n < 1 or n >= 2^31 - 16, n_sn < 0, a star outside [0, n), mass_displaced not
 * positive and finite, and cap < sum(sel_count): the error text names the size needed and NO output is written.      */
#define SPHX_SN_LDS_CAP        4096
#define SPHX_SN_CANDIDATES     0
#define SPHX_SN_LDS_SORTS      1
#define SPHX_SN_GLOBAL_SORTS   2
#define SPHX_SN_WIDENINGS      3
#define SPHX_SN_ZERO_DISTANCE  4
#define SPHX_SN_BAD_MASS       5
#define SPHX_SN_NCOUNT         6
#define SPHX_SN_STAGES         6
int sphx_supernova_impulse(sphx_ctx* ctx, int64_t n, const double* points, const double* masses, const double* ptypes,
                           int64_t n_sn, const int64_t* supernova_pos, double mass_displaced, double kick_energy,
                           double* velocities_inout /* (n,3) or NULL */, int64_t cap, int64_t* sel_count /* int64[n_sn] */,
                           int64_t* sel_ids /* int64[cap] */, double* d_vels /* (cap,3) */, double* true_mass /* [n_sn] */,
                           double* vel /* [n_sn] */, int64_t* counts /* int64[SPHX_SN_NCOUNT] or NULL */);
/* ---- the supernova event on the resident state, N unchanged                                       drv:350-358 ----- *
 * sphx_supernova_impulse on the state as it is on the device, for the stars ids[n_sn] (particle indices of the uploaded
 * state, in the driver's order), the kicks added to the resident velocities (drv:350-352), then
 *   ct = crossing_time(neighbor, velocities, sizes, particle_type)                                     drv:357
 *   dt_event = min(dt_0 / 100, ct)                                                                     drv:358
 * with the last sphx_step's own list (sphx_state_download_neighbors), the step's radii as sizes and the KICKED
 * velocities.  The state is gathered into the caller's particle order as the phases gather it and the selection runs
 * on that copy: the bits are those of sphx_supernova_impulse and sphx_crossing_time on the downloaded state.  Only the
 * velocities are written, and only when the call succeeds: a refused call leaves the state as it was.  The insertion of
 * the new particles (drv:361-396) changes N: sphx_state_insert_rows, below.
 * Outputs as sphx_supernova_impulse's (sel_ids in the caller's order); ct, dt_event: scalars.
 * SPHX_E_STATE as sphx_state_dust_phase: no state, no step yet, incremental search, the step's list gone.
 * SPHX_E_ARG: an id outside [0, n), mass_displaced not positive and finite, cap too small (the text names the size).  */
int sphx_state_supernova_impulse(sphx_ctx* ctx, int64_t n_sn, const int64_t* ids, double mass_displaced, double kick_energy,
                                 double dt_0, int64_t cap, int64_t* sel_count /* int64[n_sn] */, int64_t* sel_ids /* int64[cap] */,
                                 double* d_vels /* (cap,3) */, double* true_mass /* [n_sn] */, double* vel /* [n_sn] */,
                                 int64_t* counts /* int64[SPHX_SN_NCOUNT] or NULL */, double* ct, double* dt_event);
/* Device time of the stages of the last sphx_supernova_impulse call on this context, from HIP events on its stream, in
 * ms and added up over its stars: ms[0] keys, ms[1] the bound (histograms, one host wait per level), ms[2] compaction,
 * ms[3] the sort, ms[4] the walk and its host wait, ms[5] true_mass, vel and the kick.  Also after
 * sphx_state_supernova_impulse (the gather, the crossing time and the write-back are not in it).  Measurement aid.  */
int sphx_sn_last_timing(sphx_ctx* ctx, double ms[SPHX_SN_STAGES]);
/* ---- the insertion of a supernova's new particles into the resident state                       drv:361-396 ----- *
 * The block of the time loop that changes N.  The host forms the few new rows (nsc.supernova_explosion, nsc:820-882, on
 * the exploding stars' rows alone); the state itself never leaves the device.
 *
 * sphx_state_download_rows: the rows with the caller ids ids[n_rows] (particle indices of the uploaded state, each once)
 * in the order given: pos, vel (n_rows,3), mass, E_internal (n_rows), f_un (n_rows,s) or NULL.  One kernel over the state:
 * every storage slot looks its id up in the sorted list by binary search (no N-sized inverse table).
 * SPHX_E_STATE: no state; f_un asked of a state without one.  SPHX_E_ARG: an id outside [0, n) or given twice.
 *
 * sphx_state_insert_rows, in the driver's order:
 *   the rows rew_ids[n_rew] get rew_mass, rew_E and the composition rows rew_f_un (n_rew,s)             drv:364-366
 *   n_app rows are appended: app_pos, app_vel (n_app,3), app_mass, app_ptype, app_E (n_app), app_f_un (n_app,s); their
 *     caller ids are N .. N + n_app - 1 in the order given (the driver appends dust, then gas), their previous radius and
 *     previous acceleration 0                                                                           drv:363, 367-372
 *   T of the new rows is 0, then T[T < t_cmb] = t_cmb over ALL rows (a NaN stays)                       drv:379-382
 *   mu_array = sum(f_un mu_specie, axis=1) / sum(f_un, axis=1), gamma_array likewise with gamma_specie, formed again for
 *     EVERY row of a state that carries its composition, in NumPy's order of the row sums (a state uploaded without
 *     f_un: for the rewritten and the new rows only, from the rows given)                               drv:393-394
 *   with drag on, the rewritten and the new rows' mean grain mass and cross-section from grain_mass, sigma_effective
 *   the search of drv:386 on the N + n_app rows (k, dist as sphx_step takes them), run as the first step's search is (no
 *     radius handed to it); its list and radii are then the step's own: sphx_state_dust_phase, sphx_state_rad_phase,
 *     sphx_state_supernova_impulse, sphx_state_download_neighbors and sphx_state_download (sizes) read them; the next
 *     sphx_step sizes its grid from this search
 *   the first step of the next sphx_step call integrates dv = a dt for every row (drv:482-485: the previous acceleration
 *     has the old shape); the step after it averages again.
 * Every per-particle buffer of the state is grown with its contents kept, only where the head-room of its allocation does
 * not already hold N + n_app rows; the host checks that each holds them before the first kernel is launched.  Until the
 * next step, densities, num_densities, visc_heat and the pressure download as zeros ("not stepped yet") and
 * sphx_state_download_species is refused.
 * SPHX_E_STATE (as sphx_state_dust_phase): no state, no step yet, incremental search, the step's list gone.
 * SPHX_E_ARG: an id outside [0, N) or given twice, s not the state's, N + n_app over 2^31 - 16, a non-finite new position
 * or table entry, drag on without grain_mass and sigma_effective.  A refused call has written nothing.
 *
 * sphx_insert_last_info: info[0] buffers reallocated, [1] rows appended, [2] rows rewritten, [3] rows whose T the clamp
 * moved (new rows included).  sphx_insert_last_timing: device time of the stages of the last sphx_state_insert_rows, ms:
 * [0] checks' upload, [1] grow, [2] the insert kernel, [3] the search.                                              */
int sphx_state_download_rows(sphx_ctx* ctx, int64_t n_rows, const int64_t* ids, double* pos, double* vel, double* mass,
                             double* E_internal, double* f_un /* or NULL */);
int sphx_state_insert_rows(sphx_ctx* ctx, int s, int64_t n_rew, const int64_t* rew_ids, const double* rew_mass, const double* rew_E,
                           const double* rew_f_un, int64_t n_app, const double* app_pos, const double* app_vel,
                           const double* app_mass, const double* app_ptype, const double* app_E, const double* app_f_un, double t_cmb,
                           const double* mu_specie /* [s] */, const double* gamma_specie /* [s] */,
                           const double* grain_mass /* [s] or NULL */, const double* sigma_effective /* [s] or NULL */, int k,
                           double dist);
int sphx_insert_last_info(sphx_ctx* ctx, int64_t info[4]);
int sphx_insert_last_timing(sphx_ctx* ctx, double ms[4]);
/* ---- the adaptive length scale and sizes, the closing block of the time loop                    drv:493-540 ----- *
 * The length scale, with v_max2 = 80000**2, qf = q / 100 = 90 / 100 as the caller's double, fill = 0.9:
 *   vel_condition_i = (vx^2 + vy^2) + vz^2            np.sum(v**2, axis=1): NumPy's order over three columns   drv:493
 *   dist_sq_i       = (x^2 + y^2) + z^2                                                                         drv:515
 *   slow_i          = vel_condition_i < v_max2        (a NaN speed is not slow)                                 drv:518
 *   M               = the number of slow rows                                                                   drv:521
 *   max_dist        = np.percentile(dist_sq[slow], q), method linear:                                           drv:518
 *                       vi = (M - 1) qf, lo = floor(vi), g = vi - lo; vi >= M - 1: lo = hi = M - 1, else hi = lo + 1
 *                       a, b the order statistics of rank lo, hi; a + (b - a) g, and b - (b - a)(1 - g) where g >= 0.5
 *                       NaN when any slow row's dist_sq is NaN
 *   V_new = max_dist**(3./2.)                                                                                   drv:520
 *   d     = (V_new / M / fill * n_int)**(1./3.)       n_int: N_INT_PER_PARTICLE                                 drv:521
 * Not formed: the six coordinate percentiles of drv:495-504 and min_dist (drv:517), dead in the driver.
 * The device produces M, n_nan and the two exact order statistics a, b (integer histograms over the keys' bits: the same
 * bits on every run and in every row order); the lerp and the two pow calls run in host C in the order above, each
 * operation separately rounded (sphx_length_scale_finish, which takes no
 * context and needs no device).
 * Ours, where the driver leaves it open:
 *   1. M = 0: np.percentile raises IndexError; SPHX_E_ARG here, nothing written.
 *   2. A NaN dist_sq among the slow rows: max_dist and d are NaN, as NumPy gives; the rows are counted (n_nan), a NaN
 *      orders last (b, and a, may be NaN).  sphx_state_length_scale refuses to apply a NaN d.
 * Outputs (each but d may be NULL): n_slow = M, n_nan, lo, a, b, max_dist, d.
 * SPHX_E_ARG: a NULL required pointer, n < 1 or n >= 2^31 - 16, qf outside [0, 1], a NaN v_max2, n_int or fill, M = 0.
 *
 * The reverse counts and the adaptation:
 *   exp_neighbor_count_i = the number of entries of the whole list equal to i                                drv:527-530
 *   num_nontrivial_i     = the number of entries of row i's list inside [0, n)                               nsc:545
 *   densities_0 given (the driver: it has n rows):                                                           drv:532-533
 *     new_smoothing_i = (exp(nan_to_num(-(rho_i - rho0_i) / (3 rho_i))) * 2) / 2. + (cnt_i + nontriv_i - 1 < 2) * 0.1
 *   densities_0 NULL (the driver: another length - the first pass, the pass behind an insertion):            drv:534-535
 *     new_smoothing = 1.                                (no bonus either)
 *   sizes[ptype == 0] = (new_smoothing * sizes)[ptype == 0]                                                  drv:536
 *   sizes[(ptype == 0) & (sizes > d)] = d                                                                    drv:537
 *   sizes[ptype == 2] = d_dust                          d_dust = d / raise_factor**(1./3.), formed by the caller   drv:538
 *   densities_0 = densities                             the caller's (sphx_state_length_scale: kept)         drv:540
 * nan_to_num is NumPy's (NaN -> 0, +-inf -> +-DBL_MAX); exp is the device library's double exp (within a few ulp of
 * NumPy's); stars keep their size; a NaN size stays NaN (NaN > d is false).
 * Ours: an entry outside [0, n) is ignored (the driver's np.unique would give an array of another length and fail on the
 * broadcast) and counted; a row that nobody lists counts 0 (the driver's arrays would misalign; the step's lists hold
 * every row itself).
 * Outputs: sizes_out (n); rev_count_out, nontrivial_out int64[n], new_smoothing_out (n), each or NULL; counts
 * int64[SPHX_SCALE_NCOUNT] or NULL: rows (of any type) with the bonus, gas rows capped at d, rows (of any type) whose
 * nan_to_num changed something, missing entries.
 * SPHX_E_ARG: a NULL required pointer, n < 1 or n >= 2^31 - 16, k < 1 or k > 64.
 *
 * sphx_state_length_scale: both on the state as the last sphx_step left it - the resident positions and velocities, the
 * step's own list (sphx_state_download_neighbors), its radii as sizes, its densities (sphx_state_download's rho); nothing
 * is gathered into the caller's order.  The bits are those of the two array calls on the downloaded state.  densities_0
 * is kept on the device by particle id from one applied call to the next; sphx_state_upload and sphx_state_insert_rows
 * drop it, and the next call then takes the new_smoothing = 1. branch (as drv:532 does behind drv:368); so does a call
 * behind an insertion and before the next step, whose densities have the old row count (it keeps no densities_0).
 * apply = 1: the adapted sizes are kept resident beside the step's radii (never IN them: the hinted search reads those)
 * and are what sphx_state_dust_phase, sphx_state_rad_phase, sphx_state_rad_transfer and the crossing time of
 * sphx_state_supernova_impulse take as sizes until the next sphx_step, whose search replaces them (drv:437); densities_0
 * becomes the step's densities; with loop forms on, d becomes their d for the next step (nsc.d = d, drv:523).  Every
 * applied call starts from the step's radii: one call per pass of the loop.
 * apply = 0 writes nothing resident (densities_0 included).  sphx_state_download keeps returning the radii as sizes;
 * sphx_state_download_sizes returns the adapted ones (SPHX_E_STATE when none stand).
 * Outputs as above, d_dust = d / raise_factor**(1./3.); sizes_out (n), rev_count_out int64[n] in the caller's order, or NULL.
 * SPHX_E_STATE as sphx_state_dust_phase: no state, no step yet, incremental search, the step's list gone.
 * SPHX_E_ARG as sphx_length_scale, a NaN raise_factor, and with apply = 1 a NaN d (with loop forms on: a d that is not > 0).
 * A refused call leaves everything as it was.
 *
 * sphx_scale_last_timing: device time of the stages of the family's last call on this context, from HIP events on its
 * stream, in ms: [0] keys (array call: with the upload), [1] the selection and its one read-back, [2] the reverse counts,
 * [3] the adaptation, [4] the outputs coming back.  A stage a call does not have reads 0.  Measurement aid.         */
#define SPHX_SCALE_NCOUNT      4
int sphx_length_scale_finish(int64_t n_slow, int64_t n_nan, double qf, double a, double b, double n_int, double fill,
                             double* max_dist, double* d);
int sphx_length_scale(sphx_ctx* ctx, int64_t n, const double* points, const double* velocities, double v_max2, double qf,
                      double n_int, double fill, int64_t* n_slow, int64_t* n_nan, int64_t* lo, double* a, double* b,
                      double* max_dist, double* d);
int sphx_adapt_sizes(sphx_ctx* ctx, int64_t n, int k, const int64_t* neighbor, const double* densities,
                     const double* densities_0 /* or NULL */, const double* sizes, const double* ptype, double d, double d_dust,
                     double* sizes_out, int64_t* rev_count_out /* int64[n] or NULL */, int64_t* nontrivial_out /* int64[n] or NULL */,
                     double* new_smoothing_out /* (n) or NULL */, int64_t* counts /* int64[SPHX_SCALE_NCOUNT] or NULL */);
int sphx_state_length_scale(sphx_ctx* ctx, double v_max2, double qf, double n_int, double fill, double raise_factor, int apply,
                            int64_t* n_slow, int64_t* n_nan, int64_t* lo, double* a, double* b, double* max_dist, double* d,
                            double* d_dust, int64_t* counts /* int64[SPHX_SCALE_NCOUNT] or NULL */, double* sizes_out /* (n) or NULL */,
                            int64_t* rev_count_out /* int64[n] or NULL */);
int sphx_state_download_sizes(sphx_ctx* ctx, double* sizes);
int sphx_scale_last_timing(sphx_ctx* ctx, double ms[5]);
/* ---- the census, the ordered selections and the stellar clock    drv:244, 339-342, 465-468, 604, 616-622, 636, 656-664 -- *
 * What decides a pass of the loop (which stars explode) and what a run reports and saves, formed on the device: only a
 * few dozen numbers and the selected rows come back.  Nothing here changes N or the step; the state is only read.
 *
 * sphx_census: totals[13 + 3 s] are sums over all n rows of a per-row term; a row outside a quantity's mask contributes
 * +0.0 by selection, so a NaN of a dust row never reaches a gas sum (the reference's boolean indexing):
 *   [0..3]   mass over ptype == 0, == 1, == 2 and != 2 (the last is drv:616's denominator, a sum of its own)
 *   [4]      mass over all rows (drv:636)
 *   [5..7]   mass * total_accel_c,  [8..10] mass * velocity_c,  [11] mass * ((vx^2 + vy^2) + vz^2),  [12] E_internal
 *            (the quantities of drv:465-468 and of a kinetic / internal energy; the caller halves [11])
 *   [13 + ty s + t]   ((f_un[i,t] mu_specie[t]) / rowsum_i) * mass_i over ptype == ty: gas_, star_, dust_mass_by_species of
 *            drv:656-658, rowsum_i = np.sum(f_un[i] * mu_specie) in NumPy's order.  A row of the type with rowsum 0 gives
 *            NaN and poisons that type's sums, as in the reference.  drv:637 prints the gas quantity with the
 *            multiplication by the mass BEFORE the division: other roundings; it is not formed separately.
 * velocities, total_accel, E_internal NULL: their terms are formed from zeros.  f_un NULL: s counts as 0, 13 totals.
 * counts[4]: the rows with ptype == 0, == 1, == 2, != 2 (drv:617), exact.  max_star_mass: the largest mass over ptype == 1
 * (drv:341), a NaN among them handed on, -inf when there is no star.
 * Order of every sum: by PARTICLE ID in the order of the library's ordered totals - chunks of 256 consecutive ids, each
 * summed left to right; lane l of 256 adds the chunks l, l + 256, ... in order; then a binary tree over the lanes.  Masked
 * rows stay in their place as +0.0 (the chunks are over all n ids).  So the totals are the same bits on every call and
 * do not depend on the order the state is stored in, which changes every step.  No floating-point atomics.
 *
 * sphx_state_census: the same on the resident state (mass, ptype, the velocities, the previous total acceleration,
 * E_internal, and with mu_specie not NULL the resident f_un).  The bits are those of sphx_census on the downloaded state.
 * SPHX_E_STATE: no state; mu_specie given for a state that carries no composition.
 *
 * sphx_census_select / sphx_state_census_select: the rows with ptype == type - with window != 0 also lo < mass / unit < hi
 * (drv:660) - in ASCENDING PARTICLE ID: ids int64, their mass, T, star_ages and (f_out not NULL) f_un rows.  *count is
 * always written; ids NULL: the count alone.  The count is checked against cap, the rows the outputs hold, on the host
 * before anything is copied (SPHX_E_ARG).  T or star_ages NULL (array call): zeros.  Resident: age_out needs the ages
 * set, f_out a composition (SPHX_E_STATE).
 *
 * The stellar clock.  star_ages (n) is kept resident BY PARTICLE ID, beside the state, not in it.
 *   sphx_state_set_star_ages       ages (n) in the caller's order; NULL drops them
 *   sphx_state_download_star_ages  the same array back
 *   sphx_state_advance_star_ages   drv:604: ages[(ptype == 1) & (ages > -2)] += dt
 *   sphx_advance_star_ages         drv:604 on arrays, star_ages in place
 * sphx_state_insert_rows extends set ages by -2 for every appended row (drv:371); sphx_state_upload drops them.  A state
 * without ages behaves as it did.  SPHX_E_STATE: no state; download or advance before the ages are set.
 * The schedule (drv:244, 339-342) divides by a lifetime with pow inside and compares with 1: the device selects the star
 * rows (sphx_state_census_select, type 1) and the caller evaluates the ratio on those few rows with the reference's own
 * expression, which gives the reference's bits.  Gas rows (age -1) and inserted rows (-2) can never pass the test, so the
 * restriction to ptype == 1 changes nothing in supernova_pos.
 *
 * sphx_census_last_timing: device time of the stages of the last sphx_census / sphx_state_census on this context, in ms:
 * [0] inputs on the device (resident: the id -> slot map), [1] the chunk sums, [2] the totals, [3] the read-back.       */
int sphx_census(sphx_ctx* ctx, int64_t n, int s, const double* mass, const double* ptype, const double* f_un /* (n,s) or NULL */,
                const double* mu_specie /* (s) with f_un */, const double* velocities /* (n,3) or NULL */,
                const double* total_accel /* (n,3) or NULL */, const double* E_internal /* (n) or NULL */,
                double* totals /* (13 + 3 s) */, int64_t counts[4] /* or NULL */, double* max_star_mass /* or NULL */);
int sphx_state_census(sphx_ctx* ctx, const double* mu_specie /* (s) or NULL: 13 totals */, double* totals, int64_t counts[4],
                      double* max_star_mass);
int sphx_census_select(sphx_ctx* ctx, int64_t n, int s, const double* mass, const double* ptype, const double* T, const double* star_ages,
                       const double* f_un, int type, int window, double unit, double lo, double hi, int64_t cap, int64_t* count,
                       int64_t* ids, double* mass_out, double* T_out, double* age_out, double* f_out);
int sphx_state_census_select(sphx_ctx* ctx, int type, int window, double unit, double lo, double hi, int64_t cap, int64_t* count,
                             int64_t* ids, double* mass_out, double* T_out, double* age_out, double* f_out);
int sphx_state_set_star_ages(sphx_ctx* ctx, const double* star_ages);
int sphx_state_download_star_ages(sphx_ctx* ctx, double* star_ages);
int sphx_state_advance_star_ages(sphx_ctx* ctx, double dt);
int sphx_advance_star_ages(sphx_ctx* ctx, int64_t n, double* star_ages, const double* ptype, double dt);
int sphx_census_last_timing(sphx_ctx* ctx, double ms[4]);
/* ---- the projected maps: the state integrated along a line of sight onto a pixel grid       drv:563-597 ----- *
 * The driver draws the cloud every pass (gas by log T, dust by its temperature, stars by mass, in the y-z plane).  What
 * stands behind such a picture is the projection, formed here on the device: column density of gas and of dust and the
 * column-weighted temperature of both, at the centres of n_u x n_v pixels.
 *
 * The image.  axes = (a_u, a_v), two different coordinate indices; the line of sight is the third.  center (c_u, c_v),
 * half_width (w_u, w_v) > 0, npix (n_u, n_v).  Pixel (i, j) has its centre at
 *     u_i = c_u - w_u + (i + 1/2) 2 w_u / n_u     (evaluated left to right),   v_j likewise.
 * Outputs are (n_v, n_u), row-major: out[j n_u + i].
 *
 * Particle k.  Footprint radius R_k = h(m_k) = (m_k/m_0)^(1/3) d for gas (type 0), sizes[k] for dust (type 2); no other
 * type has one, and such a row contributes to nothing.  With b^2 = (u_i - x_k,a_u)^2 + (v_j - x_k,a_v)^2, s = R_k^2 - b^2:
 *     sigma_k = c_k s^3 sqrt(s) for s > 0, else 0,    c_k = m_k (9/(2 pi)) / R_k^9   (formed once per particle)
 * - the poly6 weight of Weigh2 (nsc:673-681) integrated along the line of sight: the integral of (R^2 - b^2 - z^2)^3 over
 * the chord is (32/35)(R^2 - b^2)^(7/2), times 315/(64 pi).
 * depth = (lo, hi), or NULL: only particles whose line-of-sight coordinate lies in [lo, hi) count.
 * A gas or dust row with a NaN or infinite coordinate (any of the three), mass or radius, or with R_k <= 0, contributes
 * to nothing and is counted in *skipped (whatever the depth says).
 *
 * The fields, per pixel:
 *   gas_column        sum of sigma_k over the gas rows with s > 0
 *   dust_column       the same over the dust rows
 *   gas_temperature   sum(sigma_k T_k) / sum(sigma_k) over the gas terms with sigma_k T_k > 0 (temperature_arb's mask,
 *                     nsc:1474-1480: a negative T drops out as it does in sphx_arb_fields); 0 where the denominator is 0
 *   dust_temperature  sum(sigma_k T_k) / sum(sigma_k) over the dust terms with sigma_k > 0; 0 where the denominator is 0
 *   count (int64)     the gas and dust rows with s > 0 at the pixel
 * Every sum runs in ASCENDING PARTICLE ID: the same bits on every call, whatever order the state is stored in.  No
 * floating-point atomics.  Any output pointer may be NULL; a NULL output's sums are not formed, the others keep their bits.
 * *pairs: the (particle, tile) pairs the call listed - the image is cut into tiles of 16 x 16 pixels, and a particle is
 * listed in the tiles that hold a pixel with |u_i - x_u| <= R_k and |v_j - x_v| <= R_k (decided on the pixel centres
 * themselves: a disc between centres lists nothing); a tile evaluates its whole list at each of its 256 pixels.  More
 * than 2^31 - 1 pairs, or a failed allocation: SPHX_E_NOMEM and nothing is written (a window far inside a cloud of wide
 * particles: project a narrower depth, or fewer pixels).
 * SPHX_E_ARG: a NULL required pointer, n < 1 or n >= 2^31 - 16, equal or out-of-range axes, a half-width that is not
 * positive and finite, a non-finite centre, n_u or n_v < 1, n_u n_v > 2^28, lo >= hi (or a NaN among them).
 *
 * sphx_project_maps: arrays in (points (n,3), the others (n)), maps out.
 * sphx_state_project: the same on the resident state - the positions, masses, types, T and sizes sphx_state_sample reads
 * (sizes: the step's radii).  SPHX_E_STATE before the first sphx_step.  The bits are those of sphx_project_maps on the
 * downloaded state.  The state is only read, in buffers of the call's own: the loop is not disturbed.
 * sphx_map_last_timing: device time of the stages of the last of the two calls on this context, in ms: [0] inputs on the
 * device (resident: the id -> slot map) and the footprints, [1] counts per tile, their scan and the pair count on the
 * host, [2] the tile lists filled and sorted, [3] the tile kernel, [4] the read-back.                                   */
int sphx_project_maps(sphx_ctx* ctx, int64_t n, const double* points, const double* mass, const double* particle_type,
                      const double* sizes, const double* T, double d, const int axes[2], const double center[2],
                      const double half_width[2], const int npix[2], const double* depth /* (lo, hi) or NULL */,
                      double* gas_column, double* dust_column, double* gas_temperature, double* dust_temperature,
                      int64_t* count, int64_t* skipped, int64_t* pairs);
int sphx_state_project(sphx_ctx* ctx, double d, const int axes[2], const double center[2], const double half_width[2],
                       const int npix[2], const double* depth, double* gas_column, double* dust_column,
                       double* gas_temperature, double* dust_temperature, int64_t* count, int64_t* skipped, int64_t* pairs);
int sphx_map_last_timing(sphx_ctx* ctx, double ms[5]);
/* ---- nsc.chemisputtering_2(points, neighbor, mass, f_un, mu_array, sizes, T, particle_type)      nsc:1265-1416 ----- *
 * Thermal / chemical sputtering of the dust rows and reuptake by the gas entries of their lists, on the list `neighbors`
 * returned (drv:405).  The module globals d and dt are arguments, and so are the per-species tables (nsc:41-52).
 *   num[i,t] = f_un[i,t] mass_i / sum_t(f_un[i,t] mu_specie[t])                             nsc:1266-1267
 * A dust row j (type_j == 2), its list entries p = neighbor[j,k]:
 *   w_k = v [v > 0] [type_p == 0], v = Weigh2(x_p, x_j, m_p, d) / mu_p                      nsc:1284, 1290
 *   the row contributes if it has a gas entry and sum_k w_k > 0                             nsc:1274, 1298
 *   scd_t = (sum_k w_k f_un[p,t]) mu_specie[t];  T_sph = sum_k w_k T_p / sum_k w_k (a star's T is 2.73)
 *   dc_t = Weigh2_dust(0; m_j, sizes_j) f_un[j,t] mu_specie[t]                              nsc:1296, 1303
 *   J_t = -diff(mrn^-0.5) / diff(mrn^0.5) / (3 mineral_densities[t]) sqrt(k_B T_sph / (2 pi mu_specie[t] amu))
 *   Y_H = min(max(0.5 exp(-4600 / T_sph), 1e-7), 1e-3) yields[t] / max(yields), Y_He the same with 5, 1e-6, 1e-2
 *   sput_t = (scd_3 / mu_3 Y_H + scd_4 Y_He / mu_4) mu_specie[t], then min(sput_t, dc_t)     nsc:1311-1316
 *   K = scd + dc - sput;  E = exp(K J dt);  L = scd + dc E - sput;  F = K / L E;  NaN -> 1;  F < 0.01 -> 0.01;
 *   F_t = 1 for t < 6                                                                        nsc:1317-1326
 *   reuptake weight wk_k (one number per entry, the same in every column >= 6, 0 below): w_k f_un[p,5] mu_specie[5] on
 *   the entries with w_k > 0, divided by its sum over them, divided by the sum again; if the sum of all of it is below
 *   1e-15 a NaN becomes 1 / (number of such entries), else 0; divided by its sum once more; nan_to_num   nsc:1336-1363
 *   new0_t = (F_t - 1) num[j,t]                                                             nsc:1374
 * and then, in ascending j, with the counts as the earlier rows left them:
 *   loss_kt = new0_t wk_k;  clamp 1: num[p,t] - loss_kt < 0.01 num[p,t] -> 0.99 num[p,t];  clamp 2: num[p,t] < 0 ->
 *   num[p,t] (both on every entry of the list, dust and star entries and j itself included, where loss = 0)
 *   sum_t = sum_k loss_kt;  clamp 3: sum_t + num[j,t] < 0.01 num[j,t] -> -0.99 num[j,t]      nsc:1382-1387
 *   num[p,t] += nan_to_num(-sum_t wk_k);  num[j,t] += sum_k nan_to_num(sum_t wk_k)          nsc:1388-1395
 * Closing correction per column t (nsc:1400-1409): pos = the sum of the positive, neg of the negative counts; if
 * neg < 0 the negative ones become 0 and the positive ones are multiplied by 1 + neg / pos.  Then
 *   mass_new_i = sum_t num[i,t] mu_specie[t],  f_un_new[i,t] = num[i,t] / sum_t num[i,t].
 * Quirks of the reference kept on purpose:
 *   1. mu_array (the input) divides the weight; the recomputed sum(f_un mu_specie) divides the counts.
 *   2. The reuptake weight is the He++ column (5) of the entry, for every species.
 *   3. The weight is normalised twice, and once more after its NaNs are filled.
 *   4. F of column 6 (e-) is computed, not masked.
 *   5. exp overflow gives inf / inf = NaN, hence F = 1.
 *   6. The final losses sum_t wk_k are not clamped again: counts may go negative, and only the closing correction
 *      removes that.
 *   7. Columns 3, 4, 5 and "the first 6" are fixed, as there; hence s >= 7.
 * Ours: double throughout where the reference holds the losses in longdouble (the difference is inside the bounds of
 * tests/chem_oracle.py).  A list entry outside [0, n) contributes nothing.  Only gas entries get a weight: the
 * reference's NaN x False = NaN of a non-gas entry with non-finite data does not arise.  A row is taken to hold distinct
 * indices.  rel_w2g, rel_w2d and w2d of the reference are dead code and are not formed.
 * The order dependence is a DAG over the dust rows (j depends on j' < j where they share a list entry); it is solved by
 * rounds: every row clamps against counts formed from the previous round's clamped sums of the earlier rows, taken in
 * ascending (j, k) from a reverse list per gas particle (4 bytes per pair, sorted), until a round changes no bit - the
 * sequential result, reached after at most (contributing rows + 1) rounds.  No floating-point atomic and no
 * waiting between workgroups: the same inputs give the same bits on every call.
 * Outputs: mass_new (n), f_un_new (n,s); counts int64[7] or NULL: contributing rows; (contributing row, gas entry)
 * pairs; clamp-1, clamp-2, clamp-3 events of the last round over (entry, column >= 6); columns corrected; rounds.
 * SPHX_E_ARG: a NULL required pointer, n < 1, k < 1 or k > 64, s < 7 or s > SPHX_MAX_SPECIES, a non-finite d, dt,
 * constant or table entry, n k beyond 2^31.
 * SPHX_CHEM_WG: lanes of a workgroup of its kernels.                                                                */
#define SPHX_CHEM_WG              256
int sphx_chemisputtering_2(sphx_ctx* ctx, int64_t n, int k, int s, const double* points, const int64_t* neighbor,
                           const double* mass, const double* f_un, const double* mu, const double* sizes, const double* T,
                           const double* ptype, double d, double dt, const double* mu_specie /* [s] */,
                           const double* mineral_densities /* [s] */, const double* sputtering_yields /* [s] */,
                           const double mrn[2], double k_B, double amu, double m_0, double* mass_new, double* f_un_new,
                           int64_t* counts /* int64[7] or NULL */);
/* Device time of the last sphx_chemisputtering_2 call on this context, from HIP events on its stream, in ms: ms[0] inputs
 * going up, records and the K-major list, ms[1] the row passes, ms[2] the reverse list (count, scan, one host wait, fill,
 * sort), ms[3] the rounds (one host wait each), ms[4] the closing correction and the outputs coming back.  Measurement
 * aid; replaces nothing in the reference.                                                                         */
int sphx_chem_last_timing(sphx_ctx* ctx, double ms[5]);
/* ---- the dust phase of the time loop, code_running.py:399-435 --------------------------------------------------- *
 * sphx_dust_bookkeeping: drv:412-433 on arrays.  mass and f_un are chemisputtering_2's outputs, mu_array the one that
 * went INTO the phase, frac_destruction / frac_reuptake supernova_destruction's outputs.  Per particle i:
 *   delta_n[t] = nan_to_num(-frac_destruction[i,t] + frac_reuptake[i,t])                                 drv:416
 *   mass_change = nan_to_num(sum_t mass_i / mu_i delta_n[t] mu_specie[t])                                drv:417
 *   f[t] = f_un[i,t] + delta_n[t];  NaN -> 1e-15;  f[t] /= sum_t f[t]                                    drv:421-424
 *   mass_out = mass_i + mass_change;  mass_out < 0 -> crit_mass / 200                                    drv:425, 431
 *   mu_out = sum_t f[t] mu_specie[t] / sum_t f[t];  gamma_out likewise with gamma_specie                 drv:432-433
 * The driver's prints come back as numbers.  totals[6]: the sum of mass_before (NaN when mass_before is NULL: the
 * masses before chemisputtering, used for nothing else), of mass, of mass_out; mass_reduction (drv:412, negative),
 * mass_increase (drv:413), the sum of mass_change (drv:419, in kg - the driver prints solar masses).  counts int64[2]:
 * masses reset at drv:431, NaN entries filled at drv:423.  Either may be NULL.
 * Quirks kept: mass_change uses the post-chem mass with the pre-phase mu; a NaN composition entry becomes 1e-15 BEFORE the
 * row is renormalised; a reset mass is crit_mass / 200 whatever it was.  The "negative compositions" prints are not
 * reproduced; cross_array and optical_depth (drv:434-435) feed rad_heating alone and are not formed.
 * Ours: double where the driver has longdouble (f_un, delta_n: DESIGN 5.12); every sum over species runs t = 0 .. s - 1
 * one by one; sums over particles are sums of chunks of 256 in index order, the chunks added in a fixed order by one
 * workgroup: no floating-point atomic, the same bits on every call.
 * SPHX_E_ARG: a NULL required pointer, n < 1, s < 1 or s > SPHX_MAX_SPECIES, a non-finite crit_mass.               */
int sphx_dust_bookkeeping(sphx_ctx* ctx, int64_t n, int s, const double* mass, const double* mu_array, const double* f_un,
                          const double* frac_destruction, const double* frac_reuptake, const double* mass_before /* or NULL */,
                          const double* mu_specie /* [s] */, const double* gamma_specie /* [s] */, double crit_mass,
                          double* mass_out, double* f_un_out, double* mu_out, double* gamma_out, double* totals /* [6] or NULL */,
                          int64_t* counts /* int64[2] or NULL */);
/* sphx_state_dust_phase: the whole block on the step loop's resident state - the first side call that WRITES it.
 *   drv:399      every row of f_un divided by its sum
 *   drv:400      density = nsc.density (sphx_density) on the current positions, the pre-phase mass, the list and d
 *   drv:401-402  dust_density and num_dens are dead in the block: not formed
 *   drv:407-408  chemisputtering_2 on (points, list, mass, the normalised f_un, the pre-phase mu, sizes, T, ptype)
 *   drv:411      supernova_destruction on (points, velocities, list, the post-chem mass and f_un, the pre-phase mu, sizes,
 *                the density of drv:400, ptype)
 *   drv:412-433  sphx_dust_bookkeeping's arithmetic
 * Inputs are the state as the last sphx_step left it; sizes is the step's kNN radius, as sphx_state_rad_transfer takes
 * it.  THE LIST IS THE LAST STEP'S OWN neighbour list, translated to particle ids: as in the driver, where `neighbor` at
 * drv:407 is what drv:437 made in the previous pass and drv:481 has moved the points since.  A missing entry (fewer
 * than k particles) is outside [0, n), which both stages ignore.  Everything is gathered into the order of upload and the
 * two ordered stages run their rows ascending in it: every output has the bits of the array calls (sphx_density,
 * sphx_chemisputtering_2, sphx_supernova_destruction, sphx_dust_bookkeeping) on the downloaded state and
 * sphx_state_download_neighbors' list.  dt, d, the tables, crit_mass, critical_density, species_curve, the knots and
 * guard_mode are those calls' arguments; m_0 is also sphx_density's and amu also sphx_supernova_destruction's (which
 * read them from the context's constants).
 * Written: mass, mu_array, gamma_array and the composition of the resident state; with drag on also mean_grain_mass and
 * mean_cross (sphx_state_set_drag), formed from the new f_un and the per-species tables grain_mass / sigma_effective as
 * np.sum(table * f_un, axis=1) - the reference recomputes them on every net_impulse call (nsc:720-726).  Nothing else
 * of the step's is touched (T, E, positions, velocities, sizes, the list).
 * Optional outputs in the order of upload, any may be NULL: density (n), mass_chem (n), f_un_chem (n,s),
 * frac_destruction, frac_reuptake (n,s); chem_counts int64[7] and dust_counts int64[5] as the array calls define them;
 * totals[6] and book_counts int64[2] as sphx_dust_bookkeeping's (totals[0] is the sum of the masses before the phase).
 * SPHX_E_STATE: no state, no sphx_step yet (the list and sizes do not exist), incremental search on (its refreshed
 * lists are not the driver's), the step's list no longer standing (since the step a call on this context has rewritten
 * the K-major list, the processing order or the ids: an array call that uploads a list, a device-API search, an upload;
 * sphx_neighbors and the samplers leave it alone), no composition of s >= 7.
 * SPHX_E_ARG: drag on without grain_mass and sigma_effective, and what the array calls refuse.  A refused call leaves the
 * state as it was.                                                                                                  */
int sphx_state_dust_phase(sphx_ctx* ctx, double dt, double d, const double* mu_specie, const double* gamma_specie,
                          const double* mineral_densities, const double* sputtering_yields, const double mrn[2], double k_B,
                          double amu, double m_0, double crit_mass, double critical_density, const int32_t* species_curve,
                          const double knots_v[8], const double knots_c[8], const double knots_si[8], int guard_mode,
                          const double* grain_mass /* [s] or NULL */, const double* sigma_effective /* [s] or NULL */,
                          double* density, double* mass_chem, double* f_un_chem, double* frac_destruction,
                          double* frac_reuptake, int64_t* chem_counts, int64_t* dust_counts, double* totals,
                          int64_t* book_counts);
/* Device time of the last sphx_state_dust_phase call, from HIP events, in ms: ms[0] the state gathered and the list
 * translated, ms[1] the density, ms[2] chemisputtering, ms[3] supernova_destruction, ms[4] the bookkeeping, the
 * write-back and the outputs coming back.  Measurement aid.                                                        */
int sphx_phase_last_timing(sphx_ctx* ctx, double ms[5]);
/* The last sphx_step's neighbour list as (n,k) int64 in particle ids, rows in the order of upload, a missing entry n
 * (nsc.neighbors' convention).  SPHX_E_STATE as sphx_state_dust_phase's first four.                                */
int sphx_state_download_neighbors(sphx_ctx* ctx, int64_t* neighbor);
/* mass (n), f_un (n,s), mu_array (n), gamma_array (n) as they are on the device, in the order of upload; any may be
 * NULL.  SPHX_E_STATE: no state; f_un asked of a state uploaded without one.                                       */
int sphx_state_download_composition(sphx_ctx* ctx, double* mass, double* f_un, double* mu_array, double* gamma_array);
/* The per-particle drag coefficients (sphx_state_set_drag; refreshed by sphx_state_dust_phase) in the order of upload;
 * either may be NULL.  SPHX_E_STATE: no state, or drag off.                                                        */
int sphx_state_download_drag(sphx_ctx* ctx, double* mean_grain_mass, double* mean_cross);
/* ---- the radiative block of the time loop, code_running.py:247-316, its elementwise half ------------------------ *
 * Between sphx_rad_transfer (nsc:922-965) and sphx_rad_cooling (nsc:1019-1176) the driver and rad_heating do per-particle
 * arithmetic on the composition rows: these three array calls.  In all of them n_gas is the number of particles with
 * ptypes != 1 (checked on the device: SPHX_E_ARG when it differs), the order of lf2 / momentum / frac_destroyed is the
 * caller's order over those particles (what rad_heating returns), every sum over species runs t = 0 .. s - 1 one by
 * one, every operation is rounded on its own, nan_to_num is NumPy's (NaN -> 0, +-inf -> +-DBL_MAX), and the same inputs
 * give the same bits on every call (no floating-point atomic).
 *
 * sphx_rad_ionise: nsc:976-1012.  Per particle i with ptypes != 1, g its ordinal among them:
 *   n_photons = photons_per_joule lf2[g]                                                                  nsc:976
 *   mols = mass_i / sum_t (f_un[i,t] mu_specie[t] amu)                                                    nsc:977
 *   weighted_interception[t] = f_un[i,t] cross_sections[t] / sum_t (cross_sections[t] f_un[i,t])          nsc:979
 *   atoms_destroyed[t] = weighted_interception[t] frac_dest[t] n_photons;  atoms_total[t] = f_un[i,t] mols   nsc:980-981
 *   frac[t] = nan_to_num(0.99 - 0.99 exp(-nan_to_num(atoms_destroyed[t] / atoms_total[t])));
 *   atoms_total[t] / amu < 1e-10 -> 0, then atoms_total[t] / amu < 0 -> 0.99                              nsc:983-988
 *   the forward reactions with the reference's literal columns: f2 += 2 f0 frac[0]; f3 += f2 frac[2]; f4 += f1 frac[1];
 *   f5 += f2 frac[2] + f1 frac[1]; f0 -= f0 frac[0]; f1 -= f1 frac[1]; f2 -= f2 frac[2] (right sides from the old row)
 *                                                                                                         nsc:999-1007
 * and for EVERY particle, stars and dust included, the row divided by its sum (nsc:1012).  Only frac[0..2] are ever
 * read, so only those are formed: frac_dest needs s entries, of which three are used.  photons_per_joule is the scalar
 * nsc:976 multiplies lf2 by (compat.stellar_spectrum).  Outputs: f_un_new (n,s); frac_destroyed (n_gas,3) or NULL.
 * SPHX_E_ARG: a NULL required pointer, n < 1, s < 6 or s > SPHX_MAX_SPECIES, n_gas not the count.                  */
int sphx_rad_ionise(sphx_ctx* ctx, int64_t n, int s, int64_t n_gas, const double* f_un, const double* ptypes, const double* mass,
                    const double* lf2 /* [n_gas] */, const double* frac_dest /* [s] */, double photons_per_joule,
                    const double* mu_specie /* [s] */, const double* cross_sections /* [s] */, double amu, double* f_un_new,
                    double* frac_destroyed /* (n_gas,3) or NULL */);
/* sphx_rad_heat_bookkeeping: drv:258-273.  f_un is sphx_rad_ionise's output.  Per particle:
 *   mu = sum_t f mu_specie / sum_t f; gamma, cross likewise with gamma_specie, cross_sections             drv:258-260
 *   where ptypes == 0: c0 = nan_to_num(lf2[g] / E); c0 >= 0 -> c0 + 1, else exp(c0); E *= c0;             drv:263-267
 *                      T = E / (N_PART gamma k_B), N_PART = mass / (m_h mu_before)                        drv:268, 248
 *   E < t_cmb gamma mass k_B / (mu m_h) -> that; E > t_max gamma mass k_B / (mu m_h) -> that;
 *   T < t_cmb -> t_cmb; T >= t_max -> t_max (all particles; a NaN stays)                                  drv:270-273
 * Quirk kept: N_PART at drv:268 is the value of drv:248, formed with the mu_array from BEFORE the heating - mu_before is
 * an input.  The driver never defines t_max (a NameError as committed): it is an argument.  The driver's cross_sections
 * are the module's plus sigma_effective (drv:58), not the table sphx_rad_ionise takes.
 * Outputs (n each): mu_out, gamma_out, cross_out, E_out, T_out.  totals[2] or NULL: the sum of E_internal on entry and
 * of E_out (chunks of 256 in index order, the chunks in a fixed order); counts int64[4] or NULL: E raised, E lowered,
 * T raised, T lowered by the clamps.                                                                                */
int sphx_rad_heat_bookkeeping(sphx_ctx* ctx, int64_t n, int s, int64_t n_gas, const double* f_un, const double* ptypes,
                              const double* mass, const double* mu_before, const double* E_internal, const double* T,
                              const double* lf2 /* [n_gas] */, const double* mu_specie, const double* gamma_specie,
                              const double* cross_sections, double t_cmb, double t_max, double k_B, double m_h, double* mu_out,
                              double* gamma_out, double* cross_out, double* E_out, double* T_out, double* totals /* [2] or NULL */,
                              int64_t* counts /* int64[4] or NULL */);
/* sphx_rad_cool_bookkeeping: drv:283-311.  final_comp and energy are sphx_rad_cooling's; lf2 and momentum
 * sphx_rad_transfer's; E_internal and T sphx_rad_heat_bookkeeping's.  Per particle:
 *   mu, gamma, cross from final_comp as above; N_PART = mass / (m_h mu)                                   drv:283-289
 *   where ptypes == 0: c1 = nan_to_num(-(energy N_PART) / E); c1 >= 0 -> c1 + 1, else exp(c1);
 *                      c1 *= exp(-dt / cooling_timescale sqrt(T / 1e4)); E *= c1; T = E / (N_PART gamma k_B)   drv:293-298
 *   where ptypes == 2: optd = 1 - exp(-(N_PART cross) 9 / (4 pi sizes^2));
 *                      T = (lf2[g] / (optd 4 pi sizes^2 sb 1e-5 dt) + t_cmb^(1/6))^(1/6); E = N_PART k_B T gamma   drv:286-301
 *   where ptypes != 1: velocities += momentum[g]                                                          drv:303
 *   the clamps of drv:270-273 again, with the new mu and gamma                                            drv:308-311
 * Quirks kept: the sixth root with t_cmb^(1/6) inside, as written; the T in the cooling_timescale factor is the T of the
 * moment (the heating's).  cooling_timescale and t_max are undefined in the driver: arguments here.
 * Outputs: mu_out, gamma_out, cross_out, E_out, T_out (n each), vel_out (n,3); totals and counts as above.
 * SPHX_E_ARG as above, and non-finite constants or cooling_timescale == 0.                                          */
int sphx_rad_cool_bookkeeping(sphx_ctx* ctx, int64_t n, int s, int64_t n_gas, const double* final_comp, const double* energy,
                              const double* ptypes, const double* mass, const double* sizes, const double* E_internal,
                              const double* T, const double* velocities, const double* lf2 /* [n_gas] */,
                              const double* momentum /* (n_gas,3) */, const double* mu_specie, const double* gamma_specie,
                              const double* cross_sections, double dt, double t_cmb, double t_max, double cooling_timescale,
                              double sb, double k_B, double m_h, double* mu_out, double* gamma_out, double* cross_out,
                              double* E_out, double* T_out, double* vel_out, double* totals /* [2] or NULL */,
                              int64_t* counts /* int64[4] or NULL */);
/* Device time of the last of the three calls above on this context, from HIP events on its stream, in ms: ms[0] inputs
 * going up and the non-star ordinals (flags, scan, one host wait), ms[1] the row kernel, ms[2] the sums behind the totals
 * (two events back to back for sphx_rad_ionise), ms[3] the outputs coming back.  Measurement aid.               */
int sphx_radphase_last_timing(sphx_ctx* ctx, double ms[4]);
/* sphx_state_rad_phase: the whole radiative block, code_running.py:247-316 with N_RADIATIVE = 1, on the step loop's
 * resident state - the second side call that WRITES it.  In this order:
 *   1  the state gathered through its ids into the order of upload: positions, velocities, mass, mu_array, sizes (the
 *      step's kNN radius, as sphx_state_rad_transfer takes it), T, E_internal, particle_type; the step's own list
 *      translated to particle ids (as sphx_state_dust_phase does); the composition rows; cross_array = sum_t f
 *      driver_cross_sections / sum_t f (drv:434: a ratio, so the normalisation of drv:399/424 does not change it beyond
 *      rounding)
 *   2  the positions of the sources and targets, by their ids
 *   3  nsc:922-965      sphx_rad_transfer's kernels
 *   4  nsc:976-1012     sphx_rad_ionise's
 *   5  drv:258-273      sphx_rad_heat_bookkeeping's (mu_before = the resident mu_array)
 *   6  nsc:1019-1176    sphx_rad_cooling's, on the step's list, with cross_array, f_un, mu_array, T as stage 5 left them
 *   7  drv:283-311      sphx_rad_cool_bookkeeping's
 *   8  the write-back through the ids: velocities, E_internal, T, mu_array, gamma_array and the composition rows of the
 *      resident state; with drag on also mean_grain_mass and mean_cross, formed from the new f_un as
 *      sphx_state_dust_phase forms them.  Positions, mass, sizes, the list and the previous temperature behind
 *      sphx_state_download_pressure are not touched.
 * Every stage runs in the order of upload on the kernels of the array calls: every output has the bits of
 * sphx_rad_transfer, sphx_rad_ionise, sphx_rad_heat_bookkeeping, sphx_rad_cooling and sphx_rad_cool_bookkeeping chained
 * on the downloaded state and sphx_state_download_neighbors' list.  source_ids / target_ids: particle ids (the order of
 * upload) of the selected stars and the sampled non-star particles; n_dst = 0 is legal (lum_factor = 0).  The physics
 * stages read amu, solar_luminosity, c, k_B, m_h and m_0 from the context's constants, as their array calls do.
 * With no star in the state the driver skips the block (drv:243): *skipped = 1, nothing is computed or written.
 * Optional outputs in the order of upload, any may be NULL: cross_array (n), lf2 (G), momentum (G,3), extinction (G),
 * f_un_ionised (n,s), frac_destroyed (G,3), heat_out (5,n): mu, gamma, cross, E_internal, T after stage 5, energy (n) and
 * rec_array (s,n) of stage 6, cross_out (n) of stage 7; totals[3]: the sum of E_internal before, after the heating, after
 * the cooling; counts int64[8]: the four clamp counts of stage 5, then of stage 7; *n_gas_out = G.
 * SPHX_E_STATE as sphx_state_dust_phase (no state, no step yet, incremental search, the step's list gone), or no
 * composition of s >= 6.  SPHX_E_ARG: drag on without grain_mass and sigma_effective, an id outside [0, n), and what the
 * array calls refuse (no particle with ptypes == 0 among them).  A refused call leaves the state as it was.        */
int sphx_state_rad_phase(sphx_ctx* ctx, double dt, double d, int64_t n_src, const int64_t* source_ids, const double* luminosities,
                         int64_t n_dst, const int64_t* target_ids, const double* frac_dest /* [s] */, double photons_per_joule,
                         const double* mu_specie, const double* gamma_specie, const double* cross_sections,
                         const double* driver_cross_sections, double amu, double t_cmb, double t_max, double cooling_timescale,
                         double sb, double k_B, double m_h, int mode, const double* grain_mass /* [s] or NULL */,
                         const double* sigma_effective /* [s] or NULL */, double* cross_array, double* lf2, double* momentum,
                         double* extinction, double* f_un_ionised, double* frac_destroyed, double* heat_out, double* energy,
                         double* rec_array, double* cross_out, double* totals, int64_t* counts, int64_t* n_gas_out, int* skipped);
/* Device time of the last sphx_state_rad_phase call that was not skipped, from HIP events, in ms: ms[0] the state
 * gathered, the list translated, cross_array and the rays' ends, ms[1] the transfer, ms[2] ionise + heat, ms[3] the
 * cooling, ms[4] the cooling's bookkeeping, the write-back and the outputs coming back.  Measurement aid.          */
int sphx_state_radphase_last_timing(sphx_ctx* ctx, double ms[5]);
int sphx_get_stats(sphx_ctx* ctx, sphx_stats* out);
int sphx_reset_stats(sphx_ctx* ctx);

/* ---- device-pointer building blocks for spatially decomposed (multi-GPU) runs ---------- *
 * A rank holds n_total = n_owned + n_ghost particles in the caller's order, owned first
 * (ghost = copy of a particle owned by another rank, sph_code_amd/multigpu.py).  Searches
 * and sums are computed for the owned particles only; every output array has n_total rows in
 * the caller's order with the owned rows written.  Between the calls the caller fills the
 * ghost rows of h, rho and m*Pi from their owners (RCCL halo exchange), because the kernel
 * uses the NEIGHBOUR's h (nsc:587-588), rho (nsc:646) and Pi (nsc:651).  All pointers are
 * DEVICE pointers; work is queued on the context's stream (sphx_set_stream: e.g. torch's
 * current stream, so no extra synchronisation is needed).                                  */
int sphx_set_stream(sphx_ctx* ctx, void* hip_stream /* a hipStream_t; NULL = HIP's default stream */);
int sphx_reset_stream(sphx_ctx* ctx);            /* back to the context's own stream */
int sphx_sync(sphx_ctx* ctx);
/* mean smoothing length of the previous search (sets the cell size of the next grid)     */
int sphx_dev_set_mean_h(sphx_ctx* ctx, double mean_h);
/* nsc.neighbors over owned+ghost candidates, owned queries.  pos (n_total,3); hint (n_total)
 * previous h per particle or NULL; rscale <= 0: context default; h_out (n_total).          */
int sphx_dev_search(sphx_ctx* ctx, int64_t n_total, int64_t n_owned, int k, const double* pos,
                    const double* hint, double rscale, double dist, double* h_out);
/* cell order of the last sphx_dev_search: out[s] (int32, n_total) = caller index of the s-th
 * particle.  A caller that re-orders its owned arrays accordingly keeps the library's gathers
 * and scatters nearly sequential on the next step.                                            */
int sphx_dev_get_order(sphx_ctx* ctx, int64_t n_total, int32_t* out);
/* gather records; h must be complete (owned from sphx_dev_search, ghosts from their owners) */
int sphx_dev_prep(sphx_ctx* ctx, const double* pos, const double* vel, const double* mass,
                  const double* h, const double* T, const double* mu, const double* gamma,
                  const double* ptype);
/* nsc:588-619; outputs (n_total,) / (n_total,3), any may be NULL                            */
int sphx_dev_density(sphx_ctx* ctx, double* rho, double* rho_dust, double* nden, double* hydro_accel);
/* nsc:639-649 + nsc:776-786; rho_complete (n_total); ct_out: device double = min crossing
 * time over the owned gas particles, or +inf when there is none (votes are at most DBL_MAX)  */
int sphx_dev_pi(sphx_ctx* ctx, const double* rho_complete, double* Pi, double* Bw, double* ct_out);
/* nsc:651-654; Bw_complete (n_total) = m Pi [t==0]; mass (n_total)                           */
int sphx_dev_visc(sphx_ctx* ctx, const double* Bw_complete, const double* mass, double* visc_accel,
                  double* visc_heat);
/* Pairwise viscosity (sphx_set_visc_mode(ctx, 1); records from sphx_dev_prep after that call): replaces sphx_dev_pi +
 * sphx_dev_visc after sphx_dev_density.  rho_complete (n_total): ghosts' densities from their owners, injected as
 * sphx_dev_pi does; mass (n_total); outputs as sphx_dev_visc; ct_out as sphx_dev_pi.  No m Pi_j halo phase is needed.
 * Honours sphx_dev_select_blobs (interior blobs while the rho_j halo phase is in flight).  SPHX_E_STATE in mode 0, and
 * when the last sphx_dev_prep ran before the mode was set (its records carry no pairwise factor).                      */
int sphx_dev_visc_pairwise(sphx_ctx* ctx, const double* rho_complete, const double* mass, double* visc_accel,
                           double* visc_heat, double* ct_out);
/* drv:233-238 and drv:460-491 on caller-order (n,3) arrays                                   */
int sphx_dev_clamp(sphx_ctx* ctx, int64_t n, double* pos, double* vel);
/* Halo / migration plumbing of the decomposed driver (sph_code_amd/multigpu.py): particles live in
 * separate device arrays of 8-byte elements, field q being (n, widths[q]); what travels are rows of
 * W = sum(widths) elements.  All pointers are device pointers (the pointer TABLES are host arrays).
 *   pack_rows: rows[t,:] = fields[idx[t],:] for t < n            (idx NULL: identity)
 *   regroup:   fields_out[t] = fields_in[sel[t]] for t < n_sel   (sel NULL: identity),
 *              fields_out[n_sel + r] = rows[r] for r < n_rows.                                   */
int sphx_dev_pack_rows(sphx_ctx* ctx, int64_t n, const int64_t* idx, int nf, const double* const* fields,
                       const int32_t* widths, double* rows);
int sphx_dev_regroup(sphx_ctx* ctx, int64_t n_sel, const int64_t* sel, int64_t n_rows, const double* rows,
                     int nf, const double* const* fields_in, const int32_t* widths,
                     double* const* fields_out);
/* multigpu.py DistributedSim._need_map: out (G^3 bytes, device) = 1 for every cell of the coarse grid
 * (host array g_lo[3] = origin, g_cs = cubic cell edge) within floor(w_i/g_cs) + 1 cells of the cell of an
 * owned particle i (pos (n,3), w (n): device) - the cells a neighbour of i can lie in.                 */
int sphx_dev_need_map(sphx_ctx* ctx, int64_t n, const double* pos, const double* w, const double* g_lo,
                      double g_cs, int G, unsigned char* out);
/* sphx_dev_integrate with the step's verdict and dt taken on the device: red2 (device) = {1 if some rank's halo
 * was too thin, -(global minimum crossing time)}, the driver's one reduction.  red2[0] > 0.5: nothing is changed
 * (the step is redone) and *dt_out = 0; otherwise dt follows drv:222-229 (first, fixed_dt as in sphx_step) and
 * is written to dt_out (device).  The host reads verdict and dt after launching this: no round trip between
 * the sums and the update.                                                                                */
int sphx_dev_integrate_auto(sphx_ctx* ctx, int64_t n_owned, double* pos, double* vel, double* accel_old,
                            double* E_internal, double* T, const double* mass, const double* mu,
                            const double* gamma, const double* ptype, const double* hydro_accel,
                            const double* visc_accel, const double* visc_heat, const double* red2,
                            int first, double fixed_dt, double* dt_out);
/* ---- the same protocol on the LOOP FORMS of the reference's time loop (drv:451-458; multigpu.py, forms = "loop") ---- *
 * after sphx_dev_search: gather the caller's owned + ghost arrays (n_total; E_internal too: del_pressure reads the
 * neighbour's, nsc:755) and build the step's records; d = the driver's global d (drv:68).                               */
int sphx_dev_loop_prep(sphx_ctx* ctx, const double* pos, const double* vel, const double* mass, const double* T,
                       const double* mu, const double* gamma, const double* ptype, const double* E_internal, double d);
/* nsc.density, dust_density, num_dens, del_pressure (nsc:693-717,744-774) for the owned particles; h_complete (n_total):
 * owned from sphx_dev_search, ghosts from their owners (dust_density uses the neighbour's radius, nsc:711).
 * Outputs caller order, (n_total,) / (n_total,3), owned entries written, any may be NULL.                              */
int sphx_dev_loop_pass1(sphx_ctx* ctx, const double* h_complete, double* rho, double* rho_dust, double* nden, double* delp);
/* nsc.artificial_viscosity + crossing_time (nsc:776-816); rho_complete (n_total): ghosts' from their owners (nsc:803).
 * ct_out as sphx_dev_pi.                                                                                                */
int sphx_dev_loop_pass2(sphx_ctx* ctx, const double* rho_complete, double* visc_accel, double* visc_heat, double* ct_out);
/* Overlap of pass 2 with the rho_j halo phase.  The search sorts its workgroups of 128 particles ("blobs") by what they
 * need from other ranks: interior (every neighbour of its owned particles is owned), boundary, idle (ghosts only).
 * sphx_dev_loop_pass2_interior, called after sphx_dev_loop_pass1 and BEFORE the ghosts' densities have arrived, launches
 * pass 2 for the interior blobs (they read only densities pass 1 left on the device); the sphx_dev_loop_pass2 that
 * follows then runs the boundary blobs and delivers the outputs.  Returns 1 if launched, 0 if there is nothing to
 * split (LDS passes off: sphx_dev_loop_pass2 does everything), < 0 on error.  Results do not depend on the split.
 * sphx_dev_blob_split_counts: {interior, boundary, idle} blobs of the last search (a device-to-host read: diagnostics). */
int sphx_dev_loop_pass2_interior(sphx_ctx* ctx);
/* Head-room of the reach sphx_dev_reach / _reach_dt claim, limited to an absolute length `cap` (0: no limit):
 * w_i = max(h_i + min((halo + skin - 1) h_i, cap), h_i + min((halo - 1) h_i, cap) + |v_i| dt).  The driver verifies
 * every plan after the search and redoes the step if a radius outgrew its claim, so this only trades ghosts for redos. */
int sphx_dev_set_reach_cap(sphx_ctx* ctx, double cap);
/* The same overlap for hydro_update's sums.  sphx_dev_select_blobs(part): the calls of sphx_dev_prep / _density / _pi /
 * _visc that follow work on  1: the interior blobs (prep: the owned particles' records),  2: the boundary blobs (prep:
 * the ghosts' records),  0: everything (the default after every sphx_dev_search).  A pass is then called twice with the
 * same output arrays: part 1 while the halo phase it does not depend on is in flight (ghost entries of its *_complete
 * input are not read), part 2 after it.  Returns 1 if the selection is in force, 0 if there is no split (the selection
 * stays "everything": do not call a pass twice), < 0 on error. */
int sphx_dev_select_blobs(sphx_ctx* ctx, int part);
int sphx_dev_blob_split_counts(sphx_ctx* ctx, int32_t counts[3]);
/* drv:460-491 on those outputs: pressure_accel = delp / rho [gas], visc_accel = av[0].  red2 == NULL: the step `dt`;
 * else verdict and dt on the device as sphx_dev_integrate_auto (dt_out required).                                       */
int sphx_dev_integrate_loop(sphx_ctx* ctx, int64_t n_owned, double* pos, double* vel, double* accel_old,
                            double* E_internal, double* T, const double* mass, const double* mu, const double* gamma,
                            const double* ptype, const double* delp, const double* rho, const double* av_accel,
                            const double* av_heat, const double* red2, int first, double fixed_dt, double dt,
                            double* dt_out);
/* Gas-dust drag (nsc:719-742) in the decomposed step: after sphx_dev_prep; mass, ptype, mean_grain_mass, mean_cross
 * (n_total,) ghosts included -> drag_on (n_total,3; owned rows: the sum over each owned particle's dust neighbours) and
 * drag_reaction (n_total,3; EVERY row: the scatter-added reaction nsc:741 - the ghosts' rows are what their owners still
 * have to add: the driver sends them back, the reverse halo).  sphx_dev_set_drag_terms hands the completed terms
 * ((n_owned,...) arrays) to the NEXT sphx_dev_integrate / _auto / _loop call: drv:462-463,473.                        */
int sphx_dev_drag(sphx_ctx* ctx, const double* mass, const double* ptype, const double* mean_grain_mass,
                  const double* mean_cross, double* drag_on, double* drag_reaction);
int sphx_dev_set_drag_terms(sphx_ctx* ctx, const double* drag_on, const double* drag_reaction, const double* rho,
                            const double* rho_dust);
/* Self-gravity of the decomposed step (the scheme of sphx_gravity_tree_parts between ranks; device pointers, the driver
 * moves the records).  All after sphx_dev_search of the same particles and before the update:
 *   _build   gathers pos (n_total,3) and mass (n_total,) in the search's cell order into buffers of its own (rows >=
 *            n_owned - the ghosts - weigh 0: they sit in the grid but belong to their owners' pyramids) and builds the
 *            pyramid about ref[3] (host), the point every rank passes alike, inside the global bounding box.
 *   _local   accel (n_owned,3) = the field of this rank's own mass: the tree walk at ws = 1..4, the direct sum at ws = 0;
 *            softening from device memory (eps_dev) or, with eps_dev NULL, by value.
 *   _export  what every peer is to get, all peers in one call.  boxes (world,6) device: the true bounding boxes {min xyz,
 *            max xyz} of every rank's owned particles, this rank's own in row `rank`; a rank without particles has max <
 *            min and gets nothing.  cells: records of 12 doubles {M, centre - ref; Sxx Syy Szz Sxy; Sxz Syz 0 0}, parts:
 *            {x, y, z, m}; peers in rank order, concatenated.  counts (world,2) int32 device: the records each peer is to
 *            get - the WANTED numbers: nothing is written beyond cap_cells / cap_parts records, and a caller that reads a
 *            total above its capacity enlarges the buffer and calls again.  ws = 0: everything as particles.
 *   _remote  ADDS the field of the given lists to accel (n_owned,3), pos (n_owned,3): fp64, cells then particles, each
 *            in list order - the same bits whenever the lists are the same.
 * Order 1 / 2: sphx_set_gravity_order (one record layout serves both).  SPHX_E_STATE without a build for the current
 * search, and for ws > 0 under incremental search.  sphx_dev_set_gravity_accel hands the completed field ((n_owned,3), or
 * NULL for none) to the NEXT sphx_dev_integrate / _auto / _loop call: drv:448-449,477.                                 */
int sphx_dev_gravity_build(sphx_ctx* ctx, int64_t n_total, int64_t n_owned, const double* pos, const double* mass,
                           const double ref[3]);
int sphx_dev_gravity_local(sphx_ctx* ctx, int ws, double G, const double* eps_dev, double eps, double* accel);
int sphx_dev_gravity_export(sphx_ctx* ctx, int world, int rank, const double* boxes, int ws, double* cells,
                            int64_t cap_cells, double* parts, int64_t cap_parts, int32_t* counts);
int sphx_dev_gravity_remote(sphx_ctx* ctx, int64_t n_owned, const double* pos, const double* cells, int64_t ncells,
                            const double* parts, int64_t nparts, double G, const double* eps_dev, double eps,
                            double* accel);
int sphx_dev_set_gravity_accel(sphx_ctx* ctx, const double* grav);
/* Species pass (nsc:624-627) of the decomposed step: after sphx_dev_prep; f_un (n_total,nspecies), mass (n_total,) ghosts
 * included -> F (nspecies,n_total); with a table set (sphx_dev_set_agb, arguments as sphx_state_set_agb) also Z (n_total,)
 * and agb_dust (n_total,nspecies) as sphx_state_download_species defines them.  Owned entries written.                  */
int sphx_dev_set_agb(sphx_ctx* ctx, int nspecies, int nspl, const int32_t* ntx, const int32_t* nty, const double* tx,
                     const double* ty, const double* coeffs, const int32_t* mapto, double divisor,
                     const double* mu_specie, double solar_mass);
int sphx_dev_species(sphx_ctx* ctx, int nspecies, const double* f_un, const double* mass, double* F, double* Z,
                     double* agb_dust);
/* multigpu.py DistributedSim._replan: w_i = max((halo_scale + skin_frac) h_i, halo_scale h_i + |v_i| dt_last), the
 * reach an owned particle claims (h, w (n), vel (n,3): device).                                          */
int sphx_dev_reach(sphx_ctx* ctx, int64_t n, const double* h, const double* vel, double halo_scale,
                   double skin_frac, double dt_last, double* w);
/* the same with dt read from device memory (as sphx_dev_integrate_auto / _loop left it), and the send mask of a plan:
   mask[p][i] = 1 when rank p's need map (maps: (world, G^3) bytes) covers the coarse cell of owned particle i (p != rank),
   counts[p] = how many.  Both let DistributedSim plan the NEXT step's halo before the host has read this step's scalars. */
int sphx_dev_reach_dt(sphx_ctx* ctx, int64_t n, const double* h, const double* vel, double halo_scale,
                      double skin_frac, const double* dt_dev, double* w);
int sphx_dev_plan_mask(sphx_ctx* ctx, int64_t n, const double* pos, const double* g_lo, double g_cs, int G,
                       int world, int rank, const unsigned char* maps, unsigned char* mask, int64_t* counts);
/* multigpu.py DistributedSim.step, this rank's end-of-step scalars in one launch: out4 (device) =
 * { any(h_i + 2 D > w_i) ? 1 : 0,  -(*ct) (ct NULL: untouched),  max h,  mean of the h <= hclip (hclip <= 0: all) }
 * over the n_owned first entries of h and w_plan.                                                        */
int sphx_dev_step_scalars(sphx_ctx* ctx, int64_t n_owned, const double* h, const double* w_plan, double D,
                          double hclip, const double* ct, double* out4);
int sphx_dev_integrate(sphx_ctx* ctx, int64_t n_owned, double* pos, double* vel, double* accel_old,
                       double* E_internal, double* T, const double* mass, const double* mu,
                       const double* gamma, const double* ptype, const double* hydro_accel,
                       const double* visc_accel, const double* visc_heat, double dt);

#ifdef __cplusplus
}
#endif
#endif /* SPHX_H */
