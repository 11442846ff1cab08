// sphx_phase.hip - the dust phase of the reference's time loop, code_running.py:399-435, on the resident state
// (sphx_state_dust_phase), its bookkeeping as an array call (sphx_dust_bookkeeping), and the two downloads that go with
// them (sphx_state_download_neighbors, sphx_state_download_composition).  Also what the radiative phase
// (sphx_radphase.hip) and sphx_state_rad_transfer share with it: the gather of the state into caller order and the
// write-back through st.id (phase_gather_kernel, phase_back_kernel), the list's translation, the tables' check.
//
// The block, statement by statement:
//   drv:399      f_un rows divided by their sums                                     phase_normalise_kernel
//   drv:400      the loop-form density (nsc:693-702) on the current positions, the pre-phase mass, the list and d
//                                                                                    sphx_loop_density_dev (sphx_density's kernel)
//   drv:401-402  dust_density and num_dens: dead in the block (nothing below reads them) - not formed
//   drv:407-408  chemisputtering_2 on (points, list, mass, normalised f_un, pre-phase mu, sizes, T, ptype)   sphx_chem_run
//   drv:411      supernova_destruction on (points, velocities, list, post-chem mass and f_un, pre-phase mu, sizes, the
//                density of drv:400, ptype)                                          sphx_dust_run
//   drv:412-433  the bookkeeping                                                      phase_book_kernel + sphx_ordered_totals
//   drv:434-435  cross_array and optical_depth feed rad_heating alone - not kept
// THE LIST IS THE LAST STEP'S OWN (ctx->nbr: int32, K-major, storage slots, -1 = missing), translated to caller ids
// through st.id (sphx_phase_map.h).  That is what the driver does: at drv:407 `neighbor` is the list drv:437 made in the
// previous pass of the loop, and drv:481 has moved the positions since - the list is one update older than the points.
// `sizes` is st.hprev, as sphx_state_rad_transfer takes it.  Everything is gathered into the caller's particle order
// (the order of upload), in which the two ordered stages then run their rows ascending: the bits are those of the array
// calls on the downloaded state.  Only st.m, st.mu, st.gam (with drag: st.mgm, st.mcs) and the composition rows fun_id
// are written.  Writing st alone is enough: the next step's first act on the state is the permutation st -> alt
// (sphx_permute_state), which overwrites every array of alt before the two swap, and every mass-derived quantity the step
// reads - the gather records, the loop-form records with h(m), the tree's sort - is rebuilt from st by that step.
// Sums over particles: sphx_ordered_totals (sphx_side.hip).  No floating-point atomic anywhere.  Vector stores from plain
// C++ only.  Every operation separately rounded; double where the driver has longdouble.
#include "sphx_internal.h"
#include "sphx_phase_map.h"
#include <cstring>
#pragma clang fp contract(off)

#define PHASE_WG 256
// per-particle terms of the totals
enum { PQ_MPRE = 0, PQ_MCHEM, PQ_MFIN, PQ_RED, PQ_INC, PQ_CHG, PQ_RESET, PQ_FILL, PQ_N };

// ---- the state into caller order; the column of every caller id (PhaseGather, sphx_internal.h) ----
__global__ __launch_bounds__(PHASE_WG) void phase_gather_kernel(PhaseGather a) {
    const int p = blockIdx.x * PHASE_WG + threadIdx.x;
    if (p >= a.n) return;
    const int j = sphx_phase_slot(a.qorder, p);
    const size_t i = (size_t)a.id[j];
    if (a.col) sphx_phase_col_lane(a.qorder, a.id, p, a.col);   // (col[i] = p: the header's rule, replayed on the host)
    const double x = a.x[j], y = a.y[j], z = a.z[j];
    if (a.pos) { a.pos[3 * i] = x; a.pos[3 * i + 1] = y; a.pos[3 * i + 2] = z; }
    if (a.sx) { a.sx[i] = x; a.sy[i] = y; a.sz[i] = z; }
    if (a.vel) { a.vel[3 * i] = a.vx[j]; a.vel[3 * i + 1] = a.vy[j]; a.vel[3 * i + 2] = a.vz[j]; }
    a.om[i] = a.m[j]; a.omu[i] = a.mu[j]; a.oh[i] = a.h[j]; a.opt[i] = a.pt[j];
    if (a.oT) a.oT[i] = a.T[j];
    if (a.oE) a.oE[i] = a.E[j];
}
__global__ __launch_bounds__(PHASE_WG) void phase_col_kernel(int n, const int* __restrict__ qorder, const int* __restrict__ id, int* col) {
    const int p = blockIdx.x * PHASE_WG + threadIdx.x;
    if (p < n) sphx_phase_col_lane(qorder, id, p, col);
}
// lane e = (kk, i), i fastest: coalesced stores
__global__ __launch_bounds__(PHASE_WG) void phase_list_kernel(int n, int npad, int k, const int* __restrict__ nbr, const int* __restrict__ id,
                                                              const int* __restrict__ col, int* __restrict__ out) {
    const long long e = (long long)blockIdx.x * PHASE_WG + threadIdx.x;
    if (e >= (long long)k * npad) return;
    const int kk = (int)(e / npad), i = (int)(e - (long long)kk * npad);
    out[e] = sphx_phase_entry(nbr, id, col, n, npad, kk, i);
}
__global__ __launch_bounds__(PHASE_WG) void phase_list64_kernel(int n, int npad, int k, const int* __restrict__ list, long long* __restrict__ out) {
    const long long e = (long long)blockIdx.x * PHASE_WG + threadIdx.x;
    if (e < (long long)n * k) out[e] = sphx_phase_entry64(list, n, npad, k, e);
}

// drv:399: the rows of fun_id (sp doubles apart) divided by their sums, into dense rows of s
__global__ __launch_bounds__(PHASE_WG) void phase_normalise_kernel(int n, int s, int sp, const double* __restrict__ fun_id, double* __restrict__ out) {
    const int i = blockIdx.x * PHASE_WG + threadIdx.x;
    if (i >= n) return;
    const double* f = fun_id + (size_t)i * sp;
    double tot = f[0];
    for (int t = 1; t < s; ++t) tot += f[t];
    for (int t = 0; t < s; ++t) out[(size_t)i * s + t] = f[t] / tot;
}

// ---- drv:412-433, one particle per lane ----
struct PhaseBook {
    int n, s, so;                                    // so: doubles between two rows of f_out
    const double *m, *mu, *f, *destr, *reup;         // post-chem mass, pre-phase mu, post-chem f_un (n,s), the fractions (n,s)
    const double* m_before;                          // pre-phase mass for the totals (nullable)
    const double *mus, *gam;                         // mu_specie, gamma (s each)
    const double *gm, *se;                           // grain_mass, sigma_effective (s each; nullable: no drag terms)
    double crit_mass;
    double *m_out, *f_out, *mu_out, *gam_out, *mgm_out, *mcs_out;
    double* pp;                                      // (PQ_N, n): the totals' per-particle terms
};
__global__ __launch_bounds__(PHASE_WG) void phase_book_kernel(PhaseBook a) {
    const int i = blockIdx.x * PHASE_WG + threadIdx.x;
    if (i >= a.n) return;
    const size_t n = (size_t)a.n;
    const double mi = a.m[i];
    const double r = mi / a.mu[i];                                           // mass / mu_array                  drv:412
    const double *de = a.destr + (size_t)i * a.s, *re = a.reup + (size_t)i * a.s, *f = a.f + (size_t)i * a.s;
    double* fo = a.f_out + (size_t)i * a.so;
    double red = 0.0, inc = 0.0, chg = 0.0, tot = 0.0;
    int fills = 0;
    for (int t = 0; t < a.s; ++t) {
        const double mst = a.mus[t];
        const double dn = sphx_nan_to_num(-de[t] + re[t]);                   // drv:416
        const double tr = r * de[t] * mst, ti = r * re[t] * mst, tc = r * dn * mst;
        red = t ? red + tr : tr; inc = t ? inc + ti : ti; chg = t ? chg + tc : tc;   // drv:412, 413, 417
        double v = f[t] + dn;                                                // drv:421
        if (v != v) { v = 1e-15; ++fills; }                                  // drv:423
        fo[t] = v;
        tot = t ? tot + v : v;
    }
    chg = sphx_nan_to_num(chg);                                              // drv:417
    double smu = 0.0, sg = 0.0, sf = 0.0;
    for (int t = 0; t < a.s; ++t) {
        const double v = fo[t] / tot;                                        // drv:424
        fo[t] = v;
        const double tm = v * a.mus[t], tg = v * a.gam[t];
        smu = t ? smu + tm : tm; sg = t ? sg + tg : tg; sf = t ? sf + v : v;
    }
    double mo = mi + chg;                                                    // drv:425
    const bool reset = mo < 0.0;
    if (reset) mo = a.crit_mass / 200.;                                      // drv:431
    a.m_out[i] = mo;
    a.mu_out[i] = smu / sf;                                                  // drv:432
    a.gam_out[i] = sg / sf;                                                  // drv:433
    if (a.gm) {                                                              // nsc:720-726, as Simulation forms them
        a.mgm_out[i] = phase_np_sum(a.s, [&](int t) { return a.gm[t] * fo[t]; });
        a.mcs_out[i] = phase_np_sum(a.s, [&](int t) { return a.se[t] * fo[t]; });
    }
    a.pp[PQ_MPRE * n + i] = a.m_before ? a.m_before[i] : 0.0;
    a.pp[PQ_MCHEM * n + i] = mi; a.pp[PQ_MFIN * n + i] = mo;
    a.pp[PQ_RED * n + i] = red; a.pp[PQ_INC * n + i] = inc; a.pp[PQ_CHG * n + i] = chg;
    a.pp[PQ_RESET * n + i] = reset ? 1.0 : 0.0; a.pp[PQ_FILL * n + i] = (double)fills;
}

// the phases' new arrays from caller order back into the storage slots (PhaseBack, sphx_internal.h)
__global__ __launch_bounds__(PHASE_WG) void phase_back_kernel(PhaseBack a) {
    const int j = blockIdx.x * PHASE_WG + threadIdx.x;
    if (j >= a.n) return;
    const size_t i = (size_t)a.id[j];
    double w[3] = {0.0, 0.0, 0.0}, v[6];                     // (every load in flight before the first store)
    if (a.vel) { w[0] = a.vel[3 * i]; w[1] = a.vel[3 * i + 1]; w[2] = a.vel[3 * i + 2]; }
#pragma unroll
    for (int q = 0; q < 6; ++q)
        if (q < a.narr) v[q] = a.in[q][i];
    if (a.vel) { a.vx[j] = w[0]; a.vy[j] = w[1]; a.vz[j] = w[2]; }
#pragma unroll
    for (int q = 0; q < 6; ++q)
        if (q < a.narr) a.out[q][j] = v[q];
}

// =====================================================================================================================
// host side
// =====================================================================================================================
static unsigned phase_blocks(size_t lanes) { return sphx_blocks(lanes, PHASE_WG); }
int sphx_phase_gather(sphx_ctx* ctx, const PhaseGather& a) {
    hipLaunchKernelGGL(phase_gather_kernel, dim3(phase_blocks((size_t)a.n)), dim3(PHASE_WG), 0, ctx->stream, a);
    HIPCHK(hipGetLastError());
    return SPHX_OK;
}
int sphx_phase_back(sphx_ctx* ctx, const PhaseBack& a) {
    hipLaunchKernelGGL(phase_back_kernel, dim3(phase_blocks((size_t)a.n)), dim3(PHASE_WG), 0, ctx->stream, a);
    HIPCHK(hipGetLastError());
    return SPHX_OK;
}
int sphx_phase_check_tables(sphx_ctx* ctx, const char* who, int s, const double* gamma, const double* grain_mass,
                            const double* sigma_effective) {
    if (ctx->drag && (!grain_mass || !sigma_effective))
        return sphx_set_err(ctx, SPHX_E_ARG, "%s: drag is on: the per-species tables grain_mass and sigma_effective are needed to refresh "
                                               "mean_grain_mass and mean_cross", who);
    for (int t = 0; t < s; ++t)
        if (!sphx_finite(gamma[t]) || (ctx->drag && (!sphx_finite(grain_mass[t]) || !sphx_finite(sigma_effective[t]))))
            return sphx_set_err(ctx, SPHX_E_ARG, "%s: table entry %d must be finite", who, t);
    return SPHX_OK;
}

// ctx->phase_out (doubles): density (n) | m_out | mu_out | gam_out | mgm | mcs (n each) | f_out (n s) | pp (PQ_N n) |
// part (PQ_N nchunk) | totals (PQ_N) | tables mus, gam, gm, se (s each)
struct PhaseOut { double *dens, *m, *mu, *gam, *mgm, *mcs, *f, *pp, *part, *tot, *tab; size_t nchunk; };
static int phase_out(sphx_ctx* ctx, int64_t n, int s, PhaseOut* o) {
    const size_t nn = (size_t)n, nchunk = sphx_tot_chunks(n);
    Carve c;
    c.take(o->dens, nn); c.take(o->m, nn); c.take(o->mu, nn); c.take(o->gam, nn); c.take(o->mgm, nn); c.take(o->mcs, nn);
    c.take(o->f, nn * (size_t)s); c.take(o->pp, PQ_N * nn); c.take(o->part, PQ_N * nchunk); c.take(o->tot, PQ_N);
    c.take(o->tab, 4 * (size_t)s);
    o->nchunk = nchunk;
    return sphx_carve_into(ctx, ctx->phase_out, c);
}

// the bookkeeping kernel and the sums behind it; the totals' copy to the host is queued (phase_totals reads it after a synchronise)
static int phase_book_run(sphx_ctx* ctx, PhaseBook a, const PhaseOut& o) {
    hipLaunchKernelGGL(phase_book_kernel, dim3(phase_blocks((size_t)a.n)), dim3(PHASE_WG), 0, ctx->stream, a);
    HIPCHK(hipGetLastError());
    return sphx_ordered_totals(ctx, a.n, PQ_N, a.pp, o.part, o.tot);
}
static void phase_totals(sphx_ctx* ctx, bool has_before, double* totals, int64_t* counts) {
    double t[PQ_N];
    std::memcpy(t, ctx->pinned->scal, sizeof(t));
    if (totals) {
        totals[0] = has_before ? t[PQ_MPRE] : NAN; totals[1] = t[PQ_MCHEM]; totals[2] = t[PQ_MFIN];
        totals[3] = -t[PQ_RED]; totals[4] = t[PQ_INC]; totals[5] = t[PQ_CHG];       // drv:412: mass_reduction carries the sign
    }
    if (counts) { counts[0] = (int64_t)t[PQ_RESET]; counts[1] = (int64_t)t[PQ_FILL]; }
}
static_assert(PQ_N <= SC_NSLOTS, "the totals fit the pinned scalar block");

extern "C" int sphx_dust_bookkeeping(sphx_ctx* ctx, int64_t n, int s, const double* mass, const double* mu_array, const double* f_un,
                                     const double* frac_destruction, const double* frac_reuptake, const double* mass_before,
                                     const double* mu_specie, const double* gamma_specie, double crit_mass, double* mass_out,
                                     double* f_un_out, double* mu_out, double* gamma_out, double* totals, int64_t* counts) {
    if (!ctx) return SPHX_E_ARG;
    if (n < 1 || n > 0x7FFFFFF0ll || s < 1 || s > SPHX_MAX_SPECIES)
        return sphx_set_err(ctx, SPHX_E_ARG, "sphx_dust_bookkeeping: n=%lld, s=%d (need n >= 1, 1 <= s <= %d)", (long long)n, s, SPHX_MAX_SPECIES);
    if (!sphx_finite(crit_mass)) return sphx_set_err(ctx, SPHX_E_ARG, "sphx_dust_bookkeeping: crit_mass=%g must be finite", crit_mass);
    NEED(mass); NEED(mu_array); NEED(f_un); NEED(frac_destruction); NEED(frac_reuptake); NEED(mu_specie); NEED(gamma_specie);
    NEED(mass_out); NEED(f_un_out); NEED(mu_out); NEED(gamma_out);
    HIPCHK(hipSetDevice(ctx->device));
    const size_t nn = (size_t)n, ns = nn * (size_t)s;
    PhaseOut o;
    SPHX_TRY(phase_out(ctx, n, s, &o));
    // inputs in ctx->chem_in: mass | mu | mass_before (n each) | f_un | destr | reup (n s each)
    double *d_m, *d_mu, *d_mb, *d_f, *d_de, *d_re;
    Carve c;
    c.take(d_m, nn); c.take(d_mu, nn); c.take(d_mb, nn); c.take(d_f, ns); c.take(d_de, ns); c.take(d_re, ns);
    SPHX_TRY(sphx_carve_into(ctx, ctx->chem_in, c));
    std::memcpy(ctx->phase_tab, mu_specie, (size_t)s * sizeof(double));       // (held by the context: the upload reads it)
    std::memcpy(ctx->phase_tab + s, gamma_specie, (size_t)s * sizeof(double));
    const CopyF64 us[] = {{mass, d_m, nn}, {mu_array, d_mu, nn}, {mass_before, d_mb, nn}, {f_un, d_f, ns}, {frac_destruction, d_de, ns},
                          {frac_reuptake, d_re, ns}, {ctx->phase_tab, o.tab, 2 * (size_t)s}};
    SPHX_TRY(sphx_upload_f64(ctx, us, 7));
    PhaseBook a;
    a.n = (int)n; a.s = s; a.so = s;
    a.m = d_m; a.mu = d_mu; a.f = d_f; a.destr = d_de; a.reup = d_re; a.m_before = mass_before ? d_mb : nullptr;
    a.mus = o.tab; a.gam = o.tab + s; a.gm = nullptr; a.se = nullptr;
    a.crit_mass = crit_mass;
    a.m_out = o.m; a.f_out = o.f; a.mu_out = o.mu; a.gam_out = o.gam; a.mgm_out = nullptr; a.mcs_out = nullptr;
    a.pp = o.pp;
    SPHX_TRY(phase_book_run(ctx, a, o));
    const CopyF64 ds[] = {{mass_out, o.m, nn}, {f_un_out, o.f, ns}, {mu_out, o.mu, nn}, {gamma_out, o.gam, nn}};
    SPHX_TRY(sphx_download_f64(ctx, ds, 4));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    phase_totals(ctx, mass_before != nullptr, totals, counts);
    return SPHX_OK;
}

// what the resident calls need: a state that has stepped, whose list is still the step's
int sphx_phase_need_list(sphx_ctx* ctx, const char* who) {
    if (!ctx->has_state) return sphx_set_err(ctx, SPHX_E_STATE, "%s: no state uploaded", who);
    if (ctx->step_count < 1)
        return sphx_set_err(ctx, SPHX_E_STATE, "%s before the first sphx_step: the list and sizes do not exist yet", who);
    if (ctx->use_verlet)
        return sphx_set_err(ctx, SPHX_E_STATE, "%s: not with incremental search (the refreshed lists are not the driver's list)", who);
    // (step_list_valid, not nbr_api_valid or qorder: other entry points reset those without touching the list, or touch
    //  the list and have the flag cleared again by a later search)
    if (!ctx->step_list_valid || ctx->step_list_n != ctx->n || ctx->step_list_k != ctx->k || !ctx->nbr.p || ctx->k < 1)
        return sphx_set_err(ctx, SPHX_E_STATE, "%s: the last step's list is gone (a call on this context has overwritten it since)", who);
    return SPHX_OK;
}
// ctx->phase_int: col (npad ints) | the caller-order K-major list (k npad ints)
int sphx_phase_ints(sphx_ctx* ctx, int64_t n, int k, PhaseInts* out) {
    const size_t npad = (size_t)sphx_pad64(n);
    Carve c;
    c.take(out->col, npad); c.take(out->list, (size_t)k * npad);
    return sphx_carve_into(ctx, ctx->phase_int, c);
}
// col (n ints) and the caller-order K-major list (k npad ints) into `list`
int sphx_phase_translate(sphx_ctx* ctx, int* col, bool col_done, int* list) {
    const int64_t n = ctx->n;
    const int k = ctx->k, npad = (int)sphx_pad64(n);
    const int* id = ctx->st.id.as<int>();
    if (!col_done) hipLaunchKernelGGL(phase_col_kernel, dim3(phase_blocks((size_t)n)), dim3(PHASE_WG), 0, ctx->stream, (int)n, ctx->step_qorder, id, col);
    hipLaunchKernelGGL(phase_list_kernel, dim3(phase_blocks((size_t)k * npad)), dim3(PHASE_WG), 0, ctx->stream, (int)n, npad, k,
                       ctx->nbr.as<int>(), id, col, list);
    HIPCHK(hipGetLastError());
    return SPHX_OK;
}

// the drag coefficients from dense composition rows (n,s) in caller order (the radiative phase's refresh)
__global__ __launch_bounds__(PHASE_WG) void phase_drag_kernel(int n, int s, const double* __restrict__ f, const double* __restrict__ gm,
                                                              const double* __restrict__ se, double* mgm, double* mcs) {
    const int i = blockIdx.x * PHASE_WG + threadIdx.x;
    if (i >= n) return;
    const double* fo = f + (size_t)i * s;
    mgm[i] = phase_np_sum(s, [&](int t) { return gm[t] * fo[t]; });          // nsc:720-726, as Simulation forms them
    mcs[i] = phase_np_sum(s, [&](int t) { return se[t] * fo[t]; });
}
int sphx_phase_drag_refresh(sphx_ctx* ctx, int64_t n, int s, const double* f, const double* gm, const double* se, double* mgm, double* mcs) {
    hipLaunchKernelGGL(phase_drag_kernel, dim3(phase_blocks((size_t)n)), dim3(PHASE_WG), 0, ctx->stream, (int)n, s, f, gm, se, mgm, mcs);
    HIPCHK(hipGetLastError());
    return SPHX_OK;
}

extern "C" int sphx_state_download_neighbors(sphx_ctx* ctx, int64_t* neighbor) {
    if (!ctx) return SPHX_E_ARG;
    SPHX_TRY(sphx_phase_need_list(ctx, "sphx_state_download_neighbors"));
    NEED(neighbor);
    HIPCHK(hipSetDevice(ctx->device));
    const int64_t n = ctx->n;
    const int k = ctx->k;
    const size_t npad = (size_t)sphx_pad64(n), nk = (size_t)n * (size_t)k;
    PhaseInts pi;
    SPHX_TRY(sphx_phase_ints(ctx, n, k, &pi));
    SPHX_TRY(sphx_ensure(ctx, ctx->idx64, nk * sizeof(int64_t)));
    const int* list = pi.list;
    SPHX_TRY(sphx_phase_translate(ctx, pi.col, false, pi.list));
    hipLaunchKernelGGL(phase_list64_kernel, dim3(phase_blocks(nk)), dim3(PHASE_WG), 0, ctx->stream, (int)n, (int)npad, k, list,
                       (long long*)ctx->idx64.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(neighbor, ctx->idx64.p, nk * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SPHX_OK;
}

// per-particle arrays of the state, storage order on the device, into the caller's order on the host (host NULL: skipped)
struct ById { double* host; const double* dev; };
static int phase_download_by_id(sphx_ctx* ctx, const ById* v, int nv) {
    const int64_t n = ctx->n;
    const size_t nb = (size_t)n * sizeof(double);
    SPHX_TRY(sphx_ensure(ctx, ctx->out_a, nb));
    double* stage = ctx->out_a.as<double>();
    for (int q = 0; q < nv; ++q) {
        if (!v[q].host) continue;
        SPHX_TRY(sphx_scatter_rows_by_id(ctx, n, 1, ctx->st.id.as<int>(), v[q].dev, stage));
        HIPCHK(hipMemcpyAsync(v[q].host, stage, nb, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    return SPHX_OK;
}

extern "C" int sphx_state_download_composition(sphx_ctx* ctx, double* mass, double* f_un, double* mu_array, double* gamma_array) {
    if (!ctx) return SPHX_E_ARG;
    if (!ctx->has_state) return sphx_set_err(ctx, SPHX_E_STATE, "sphx_state_download_composition: no state uploaded");
    if (f_un && (ctx->s < 1 || !ctx->fun_id.p))
        return sphx_set_err(ctx, SPHX_E_STATE, "sphx_state_download_composition: the state carries no composition (f_un)");
    HIPCHK(hipSetDevice(ctx->device));
    const int64_t n = ctx->n;
    const StateArrays& s = ctx->st;
    const ById v1[] = {{mass, s.m.as<double>()}, {mu_array, s.mu.as<double>()}, {gamma_array, s.gam.as<double>()}};
    SPHX_TRY(phase_download_by_id(ctx, v1, 3));
    if (f_un) {                                      // the rows are in upload order already; the padding stays behind
        HIPCHK(hipMemcpy2DAsync(f_un, (size_t)ctx->s * sizeof(double), ctx->fun_id.p, (size_t)ctx->sp * sizeof(double),
                                (size_t)ctx->s * sizeof(double), (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    return SPHX_OK;
}

extern "C" int sphx_state_download_drag(sphx_ctx* ctx, double* mean_grain_mass, double* mean_cross) {
    if (!ctx) return SPHX_E_ARG;
    if (!ctx->has_state || !ctx->drag) return sphx_set_err(ctx, SPHX_E_STATE, "sphx_state_download_drag: no state with drag on");
    HIPCHK(hipSetDevice(ctx->device));
    const ById v1[] = {{mean_grain_mass, ctx->st.mgm.as<double>()}, {mean_cross, ctx->st.mcs.as<double>()}};
    return phase_download_by_id(ctx, v1, 2);
}

extern "C" int sphx_state_dust_phase(sphx_ctx* ctx, double dt, double d, const double* mu_specie, const double* gamma_specie,
                                     const double* mineral_densities, const double* sputtering_yields, const double mrn[2], double k_B,
                                     double amu, double m_0, double crit_mass, double critical_density, const int32_t* species_curve,
                                     const double knots_v[8], const double knots_c[8], const double knots_si[8], int guard_mode,
                                     const double* grain_mass, const double* sigma_effective, double* density, double* mass_chem,
                                     double* f_un_chem, double* frac_destruction, double* frac_reuptake, int64_t* chem_counts,
                                     int64_t* dust_counts, double* totals, int64_t* book_counts) {
    if (!ctx) return SPHX_E_ARG;
    const char* who = "sphx_state_dust_phase";
    SPHX_TRY(sphx_phase_need_list(ctx, who));
    if (ctx->s < 7 || !ctx->fun_id.p)
        return sphx_set_err(ctx, SPHX_E_STATE, "%s: the state carries no composition (f_un) of >= 7 species", who);
    const int64_t n = ctx->n;
    const int k = ctx->k, s = ctx->s, sp = ctx->sp;
    NEED(mu_specie); NEED(gamma_specie); NEED(mineral_densities); NEED(sputtering_yields); NEED(mrn);
    NEED(species_curve); NEED(knots_v); NEED(knots_c); NEED(knots_si);
    SPHX_TRY(sphx_chem_check_shape(ctx, who, n, k, s));
    SPHX_TRY(sphx_chem_check_scalars(ctx, who, d, dt, mrn, k_B, amu, m_0));
    SPHX_TRY(sphx_dust_check_scalars(ctx, who, crit_mass, critical_density, guard_mode));
    SPHX_TRY(sphx_phase_check_tables(ctx, who, s, gamma_specie, grain_mass, sigma_effective));
    ChemPar cpar;
    cpar.d = d; cpar.dt = dt; cpar.k_B = k_B; cpar.m_0 = m_0;
    SPHX_TRY(sphx_chem_tables(ctx, who, s, mu_specie, mineral_densities, sputtering_yields, mrn, amu, &cpar.symax));
    DustPar dpar;
    SPHX_TRY(sphx_dust_params(ctx, who, s, crit_mass, critical_density, species_curve, knots_v, knots_c, knots_si, guard_mode, &dpar));
    dpar.amu = amu;
    HIPCHK(hipSetDevice(ctx->device));
    SPHX_TRY(ctx->phase_t.begin(ctx));
    hipStream_t stream = ctx->stream;
    const size_t nn = (size_t)n, ns = nn * (size_t)s;
    // ---- the state into caller order (straight into the stages' input buffers), the list into caller ids ----
    ChemDev cin;
    DustDev din;
    ChemInts ci;
    PhaseInts pi;
    PhaseOut o;
    SPHX_TRY(sphx_chem_inputs(ctx, n, s, &cin));
    SPHX_TRY(sphx_dust_inputs(ctx, n, s, &din));
    SPHX_TRY(sphx_chem_ints(ctx, n, k, &ci));
    SPHX_TRY(phase_out(ctx, n, s, &o));
    SPHX_TRY(sphx_phase_ints(ctx, n, k, &pi));
    int *list = ci.nbr, *col = pi.col;                // (the translated list goes straight into chem's place for it)
    const StateArrays& st = ctx->st;
    PhaseGather ga;
    ga.n = (int)n; ga.qorder = ctx->step_qorder; ga.id = st.id.as<int>();
    ga.x = st.x.as<double>(); ga.y = st.y.as<double>(); ga.z = st.z.as<double>();
    ga.vx = st.vx.as<double>(); ga.vy = st.vy.as<double>(); ga.vz = st.vz.as<double>();
    ga.m = st.m.as<double>(); ga.mu = st.mu.as<double>(); ga.h = sphx_phase_sizes(ctx); ga.T = st.T.as<double>(); ga.pt = st.ptype.as<double>();
    ga.E = nullptr;
    ga.col = col; ga.pos = cin.pos; ga.sx = ga.sy = ga.sz = nullptr; ga.vel = din.vel; ga.om = cin.m; ga.omu = cin.mu; ga.oh = cin.sizes;
    ga.oT = cin.T; ga.opt = cin.ptype; ga.oE = nullptr;
    SPHX_TRY(sphx_phase_gather(ctx, ga));
    hipLaunchKernelGGL(phase_normalise_kernel, dim3(phase_blocks(nn)), dim3(PHASE_WG), 0, stream, (int)n, s, sp, ctx->fun_id.as<double>(), cin.fun);
    HIPCHK(hipGetLastError());
    SPHX_TRY(sphx_phase_translate(ctx, col, true, list));
    // the tables: chem's four (ctx->chem_tab) beside its inputs; mu_specie | gamma | grain_mass | sigma_effective in phase_out
    double* ptab = ctx->phase_tab;                   // (held by the context: the upload below reads it)
    for (int t = 0; t < s; ++t) {
        ptab[t] = mu_specie[t]; ptab[s + t] = gamma_specie[t];
        ptab[2 * s + t] = ctx->drag ? grain_mass[t] : 0.0; ptab[3 * s + t] = ctx->drag ? sigma_effective[t] : 0.0;
    }
    HIPCHK(hipMemcpyAsync(cin.tab, ctx->chem_tab, 4 * (size_t)s * sizeof(double), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(o.tab, ptab, 4 * (size_t)s * sizeof(double), hipMemcpyHostToDevice, stream));
    SPHX_TRY(ctx->phase_t.mark(ctx, 1));
    // ---- drv:400 ----
    SPHX_TRY(sphx_loop_density_dev(ctx, n, k, list, cin.pos, cin.m, cin.ptype, d, m_0, o.dens));
    SPHX_TRY(ctx->phase_t.mark(ctx, 2));
    // ---- drv:407-408 ----
    ChemRes cres;
    SPHX_TRY(sphx_chem_run(ctx, who, n, k, s, cin, list, cpar, nullptr, &cres));
    HIPCHK(hipMemcpyAsync(ctx->pinned->side.red, cres.counters + 4, 4 * sizeof(double), hipMemcpyDeviceToHost, stream));
    SPHX_TRY(ctx->phase_t.mark(ctx, 3));
    HIPCHK(hipStreamSynchronize(stream));
    sphx_chem_counts(ctx, &cres, chem_counts);
    // ---- drv:411 ----
    din.pos = cin.pos; din.m = cres.mass_new; din.mu = cin.mu; din.sizes = cin.sizes; din.dens = o.dens; din.ptype = cin.ptype;
    din.fun = cres.fun_new;
    DustRes dres;
    SPHX_TRY(sphx_dust_run(ctx, who, n, k, s, din, list, dpar, nullptr, &dres));
    SPHX_TRY(ctx->phase_t.mark(ctx, 4));
    // ---- drv:412-433; the composition rows straight into fun_id ----
    PhaseBook a;
    a.n = (int)n; a.s = s; a.so = sp;
    a.m = cres.mass_new; a.mu = cin.mu; a.f = cres.fun_new; a.destr = dres.destr; a.reup = dres.reup; a.m_before = cin.m;
    a.mus = o.tab; a.gam = o.tab + s; a.gm = ctx->drag ? o.tab + 2 * s : nullptr; a.se = ctx->drag ? o.tab + 3 * s : nullptr;
    a.crit_mass = crit_mass;
    a.m_out = o.m; a.f_out = ctx->fun_id.as<double>(); a.mu_out = o.mu; a.gam_out = o.gam; a.mgm_out = o.mgm; a.mcs_out = o.mcs;
    a.pp = o.pp;
    SPHX_TRY(phase_book_run(ctx, a, o));
    const PhaseBack ba{(int)n, st.id.as<int>(), nullptr, nullptr, nullptr, nullptr, ctx->drag ? 5 : 3,
                       {o.m, o.mu, o.gam, o.mgm, o.mcs, nullptr},
                       {st.m.as<double>(), st.mu.as<double>(), st.gam.as<double>(), st.mgm.as<double>(), st.mcs.as<double>(), nullptr}};
    SPHX_TRY(sphx_phase_back(ctx, ba));
    const CopyF64 ds[] = {{density, o.dens, nn}, {mass_chem, cres.mass_new, nn}, {f_un_chem, cres.fun_new, ns}, {frac_destruction, dres.destr, ns},
                          {frac_reuptake, dres.reup, ns}, {dust_counts, dres.counters, 5}};
    SPHX_TRY(sphx_download_f64(ctx, ds, 6));
    SPHX_TRY(ctx->phase_t.mark(ctx, 5));
    HIPCHK(hipStreamSynchronize(stream));
    phase_totals(ctx, true, totals, book_counts);
    return ctx->phase_t.end(ctx);
}
