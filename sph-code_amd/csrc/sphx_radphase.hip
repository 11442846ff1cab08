// sphx_radphase.hip - the elementwise half of the radiative block of the reference's time loop, code_running.py:247-316:
// what lies between and behind rad_transfer (sphx_rad.hip, nsc:922-965) and rad_cooling (sphx_cool.hip, nsc:1019-1176).
//
//   nsc:976-1012  the photoionisation chemistry of rad_heating                      sphx_rad_ionise            rp_ionise_kernel
//   drv:258-273   mu, gamma, cross; the heating of E and T; the clamps              sphx_rad_heat_bookkeeping  rp_book_kernel<false>
//   drv:283-311   the tables again; the cooling of E and T, the dust temperature,
//                 the radiation's impulse; the clamps                               sphx_rad_cool_bookkeeping  rp_book_kernel<true>
// The per-particle formulas are sphx_radphase_pair.h's, written once for these kernels and the host replay.
//
// ROW LAYOUT.  A particle's composition is a row of s doubles; one lane reading its own row from global memory touches a
// cache line per lane and load (phase_book_kernel, DESIGN 5.13: 0.5 TB/s).  Here a workgroup of RP_WG lanes stages the
// rows of its RP_WG particles through LDS: lane e of the copy takes double e of the tile, so the global loads and stores
// are contiguous over the wave; a row sits (s | 1) doubles from the next, so that the lanes' walks along their rows
// spread over the banks.  Each lane then works on its particle's row alone, in species order: no reduction crosses
// lanes, and no result depends on the launch shape.
// Sums over particles (the totals the driver prints): sphx_ordered_totals (sphx_side.hip).  No floating-point atomic.
// Vector stores from plain C++.
#include "sphx_internal.h"
#include "sphx_radphase_pair.h"
#include <cstring>
#include <vector>
#pragma clang fp contract(off)

#define RP_WG 128
// per-particle terms of the totals: E_internal on entry and on exit, the four clamps
enum { RQ_EIN = 0, RQ_EOUT, RQ_ELO, RQ_EHI, RQ_TLO, RQ_THI, RQ_N };
static_assert(RQ_N <= SC_NSLOTS, "the totals fit the pinned scalar block");

__device__ __forceinline__ int rp_stride(int s) { return s | 1; }
// The tile's rows, dense in global memory (double e of the tile is f[base s + e]), into LDS rows of rp_stride(s) and
// back; `cnt` particles from `base`.  A lane walks e = lane, lane + RP_WG, ...: its (row, species) pair is stepped along,
// one division per lane and none per element.
struct RpWalk {
    int r, t, dr, dt;
    __device__ __forceinline__ RpWalk(int s) : r((int)threadIdx.x / s), t((int)threadIdx.x % s), dr(RP_WG / s), dt(RP_WG % s) {}
    __device__ __forceinline__ void step(int s) {
        r += dr; t += dt;
        if (t >= s) { t -= s; ++r; }
    }
};
__device__ __forceinline__ void rp_rows_in(double* sm, const double* __restrict__ f, int base, int cnt, int s) {
    const int ls = rp_stride(s);
    const double* src = f + (size_t)base * s;
    RpWalk w(s);
    for (int e = threadIdx.x; e < cnt * s; e += RP_WG, w.step(s)) sm[w.r * ls + w.t] = src[e];
}
__device__ __forceinline__ void rp_rows_out(const double* sm, double* __restrict__ f, int base, int cnt, int s) {
    const int ls = rp_stride(s);
    double* dst = f + (size_t)base * s;
    RpWalk w(s);
    for (int e = threadIdx.x; e < cnt * s; e += RP_WG, w.step(s)) dst[e] = sm[w.r * ls + w.t];
}
// `count` doubles of a table into LDS
__device__ __forceinline__ void rp_table_in(double* sm, const double* __restrict__ tab, int count) {
    for (int e = threadIdx.x; e < count; e += RP_WG) sm[e] = tab[e];
}
static size_t rp_lds_bytes(int s, int tables) { return ((size_t)RP_WG * (size_t)(s | 1) + (size_t)tables * (size_t)s) * sizeof(double); }

// flag[i] = ptype[i] != 1 for i < n, flag[n] = 0: scanned into the non-star ordinals
__global__ __launch_bounds__(256) void rp_flag_kernel(int n, const double* __restrict__ ptype, int* __restrict__ flag) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i <= n) flag[i] = (i < n && ptype[i] != 1.0) ? 1 : 0;
}

// ---- nsc:976-1012 ----
struct RpIon {
    int n, s;
    const double *f_in, *m, *pt, *lf2;              // lf2 over the non-star particles
    const int* off;                                 // ordinal of particle i among the non-star ones
    const double* tab;                              // mu_specie | cross_sections | frac_dest (s each)
    double ppj, amu;
    double *f_out, *frac;                           // frac: (G,3), nullable
};
__global__ __launch_bounds__(RP_WG) void rp_ionise_kernel(RpIon a) {
    extern __shared__ double rp_sm[];
    const int s = a.s, ls = rp_stride(s);
    const int base = blockIdx.x * RP_WG, cnt = min(RP_WG, a.n - base);
    double* tab = rp_sm + RP_WG * ls;
    rp_rows_in(rp_sm, a.f_in, base, cnt, s);
    rp_table_in(tab, a.tab, 3 * s);
    __syncthreads();
    if ((int)threadIdx.x < cnt) {
        const int i = base + threadIdx.x;
        double* f = rp_sm + threadIdx.x * ls;
        if (a.pt[i] != 1.0) {
            const int g = a.off[i];
            double fr[3];
            sphx_rp_ionise_row(s, f, a.m[i], a.lf2[g], a.ppj, tab + 2 * s, tab, tab + s, a.amu, fr);
            if (a.frac) { a.frac[3 * (size_t)g] = fr[0]; a.frac[3 * (size_t)g + 1] = fr[1]; a.frac[3 * (size_t)g + 2] = fr[2]; }
        }
        sphx_rp_normalise_row(s, f);
    }
    __syncthreads();
    rp_rows_out(rp_sm, a.f_out, base, cnt, s);
}

// ---- drv:258-273 and drv:283-311 ----
struct RpBook {
    int n, s;
    const double *f, *pt, *m, *E, *T;
    const double *mu_before;                        // heat alone
    const double *sizes, *energy, *vel, *mom;       // cool alone; mom over the non-star particles, (G,3)
    const double* lf2;                              // over the non-star particles
    const int* off;
    const double* tab;                              // mu_specie | gamma | cross_sections (s each)
    SphxRpConst c;
    double *mu_out, *gam_out, *cross_out, *E_out, *T_out, *vel_out;
    double* pp;                                     // (RQ_N, n)
};
template <bool COOL>
__global__ __launch_bounds__(RP_WG) void rp_book_kernel(RpBook a) {
    extern __shared__ double rp_sm[];
    const int s = a.s, ls = rp_stride(s);
    const int base = blockIdx.x * RP_WG, cnt = min(RP_WG, a.n - base);
    double* tab = rp_sm + RP_WG * ls;
    rp_rows_in(rp_sm, a.f, base, cnt, s);
    rp_table_in(tab, a.tab, 3 * s);
    __syncthreads();
    if ((int)threadIdx.x >= cnt) return;
    const int i = base + threadIdx.x;
    const size_t n = (size_t)a.n;
    double mu, gamma, cross;
    sphx_rp_tables(s, rp_sm + threadIdx.x * ls, tab, tab + s, tab + 2 * s, &mu, &gamma, &cross);
    const double pt = a.pt[i], m = a.m[i], e_in = a.E[i];
    double E = e_in, T = a.T[i];
    const int g = pt != 1.0 ? a.off[i] : 0;
    const double lf2 = pt != 1.0 ? a.lf2[g] : 0.0;
    int hit;
    if (COOL) {
        double v[3] = {a.vel[3 * (size_t)i], a.vel[3 * (size_t)i + 1], a.vel[3 * (size_t)i + 2]};
        double mo[3] = {0.0, 0.0, 0.0};
        if (pt != 1.0) { mo[0] = a.mom[3 * (size_t)g]; mo[1] = a.mom[3 * (size_t)g + 1]; mo[2] = a.mom[3 * (size_t)g + 2]; }
        hit = sphx_rp_cool(a.c, pt, m, a.sizes[i], a.energy[i], lf2, mo, mu, gamma, cross, &E, &T, v);
        a.vel_out[3 * (size_t)i] = v[0]; a.vel_out[3 * (size_t)i + 1] = v[1]; a.vel_out[3 * (size_t)i + 2] = v[2];
    } else {
        hit = sphx_rp_heat(a.c, pt, m, lf2, a.mu_before[i], mu, gamma, &E, &T);
    }
    a.mu_out[i] = mu; a.gam_out[i] = gamma; a.cross_out[i] = cross; a.E_out[i] = E; a.T_out[i] = T;
    a.pp[RQ_EIN * n + i] = e_in; a.pp[RQ_EOUT * n + i] = E;
    a.pp[RQ_ELO * n + i] = (hit & SPHX_RP_E_LO) ? 1.0 : 0.0; a.pp[RQ_EHI * n + i] = (hit & SPHX_RP_E_HI) ? 1.0 : 0.0;
    a.pp[RQ_TLO * n + i] = (hit & SPHX_RP_T_LO) ? 1.0 : 0.0; a.pp[RQ_THI * n + i] = (hit & SPHX_RP_T_HI) ? 1.0 : 0.0;
}

// =====================================================================================================================
// host side
// =====================================================================================================================

// (the arrays of ctx->radphase_buf and ctx->radstate_buf each start on a 16-byte boundary: RP_AL)
#define RP_AL 16

static int rp_check(sphx_ctx* ctx, const char* who, int64_t n, int s, int64_t n_gas) {
    if (n < 1 || n > 0x7FFFFFF0ll || s < 6 || s > SPHX_MAX_SPECIES)
        return sphx_set_err(ctx, SPHX_E_ARG, "%s: n=%lld, s=%d (need n >= 1, 6 <= s <= %d)", who, (long long)n, s, SPHX_MAX_SPECIES);
    if (n_gas < 0 || n_gas > n) return sphx_set_err(ctx, SPHX_E_ARG, "%s: n_gas=%lld outside [0, n]", who, (long long)n_gas);
    return SPHX_OK;
}
// the non-star ordinals of the particles (ptype on the device) into ctx->radphase_int; their number must be n_gas
// (n_gas < 0: no number is expected; *count_out, if given, receives the number found)
static int rp_ordinals(sphx_ctx* ctx, const char* who, int64_t n, const double* d_pt, int64_t n_gas, int** off_out,
                       int64_t* count_out = nullptr) {
    int *flag, *off;                                 // n + 1 entries each and four of head-room, on 16-byte boundaries
    Carve c;
    c.take(flag, (size_t)n + 5, 16); c.take(off, (size_t)n + 5, 16);
    c.pad(16);
    SPHX_TRY(sphx_carve_into(ctx, ctx->radphase_int, c));
    hipLaunchKernelGGL(rp_flag_kernel, dim3(sphx_blocks((size_t)n + 1, 256)), dim3(256), 0, ctx->stream, (int)n, d_pt, flag);
    HIPCHK(hipGetLastError());
    SPHX_TRY(sphx_excl_scan_int(ctx, flag, off, (int)n));
    PinnedSide& pin = ctx->pinned->side;
    HIPCHK(hipMemcpyAsync(&pin.count, off + n, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (count_out) *count_out = pin.count;
    if (n_gas >= 0 && pin.count != n_gas)
        return sphx_set_err(ctx, SPHX_E_ARG, "%s: %d particles have ptypes != 1, the per-particle inputs hold n_gas=%lld", who, pin.count,
                            (long long)n_gas);
    *off_out = off;
    return SPHX_OK;
}

extern "C" int sphx_rad_ionise(sphx_ctx* ctx, int64_t n, int s, int64_t n_gas, const double* f_un, const double* ptypes,
                               const double* mass, const double* lf2, const double* frac_dest, double photons_per_joule,
                               const double* mu_specie, const double* cross_sections, double amu, double* f_un_new,
                               double* frac_destroyed) {
    if (!ctx) return SPHX_E_ARG;
    const char* who = "sphx_rad_ionise";
    SPHX_TRY(rp_check(ctx, who, n, s, n_gas));
    NEED(f_un); NEED(ptypes); NEED(mass); NEED(frac_dest); NEED(mu_specie); NEED(cross_sections); NEED(f_un_new);
    if (n_gas > 0) NEED(lf2);
    HIPCHK(hipSetDevice(ctx->device));
    SPHX_TRY(ctx->radphase_t.begin(ctx));
    const size_t nn = (size_t)n, ns = nn * (size_t)s, ng = (size_t)n_gas;
    double *d_f, *d_fo, *d_pt, *d_m, *d_lf2, *d_fr, *d_tab;
    Carve b;
    b.take(d_f, ns, RP_AL); b.take(d_fo, ns, RP_AL); b.take(d_pt, nn, RP_AL); b.take(d_m, nn, RP_AL); b.take(d_lf2, ng, RP_AL);
    b.take(d_fr, 3 * ng, RP_AL); b.take(d_tab, 3 * (size_t)s, RP_AL);
    b.pad(RP_AL);
    b.slack(8 * sizeof(double));
    SPHX_TRY(sphx_carve_into(ctx, ctx->radphase_buf, b));
    double* tab = ctx->radphase_tab;                 // (held by the context: the upload reads it)
    std::memcpy(tab, mu_specie, (size_t)s * sizeof(double));
    std::memcpy(tab + s, cross_sections, (size_t)s * sizeof(double));
    std::memcpy(tab + 2 * s, frac_dest, (size_t)s * sizeof(double));
    const CopyF64 us[] = {{f_un, d_f, ns}, {ptypes, d_pt, nn}, {mass, d_m, nn}, {n_gas > 0 ? lf2 : nullptr, d_lf2, ng}, {tab, d_tab, 3 * (size_t)s}};
    SPHX_TRY(sphx_upload_f64(ctx, us, 5));
    int* off;
    SPHX_TRY(rp_ordinals(ctx, who, n, d_pt, n_gas, &off));
    RpIon a;
    a.n = (int)n; a.s = s;
    a.f_in = d_f; a.m = d_m; a.pt = d_pt; a.lf2 = d_lf2; a.off = off; a.tab = d_tab;
    a.ppj = photons_per_joule; a.amu = amu;
    a.f_out = d_fo; a.frac = frac_destroyed ? d_fr : nullptr;
    SPHX_TRY(ctx->radphase_t.mark(ctx, 1));
    hipLaunchKernelGGL(rp_ionise_kernel, dim3(sphx_blocks(nn, RP_WG)), dim3(RP_WG), rp_lds_bytes(s, 3), ctx->stream, a);
    HIPCHK(hipGetLastError());
    SPHX_TRY(ctx->radphase_t.mark(ctx, 2));
    SPHX_TRY(ctx->radphase_t.mark(ctx, 3));                                  // (no sums behind this kernel)
    const CopyF64 ds[] = {{f_un_new, d_fo, ns}, {frac_destroyed, d_fr, 3 * ng}};
    SPHX_TRY(sphx_download_f64(ctx, ds, 2));
    SPHX_TRY(ctx->radphase_t.mark(ctx, 4));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ctx->radphase_t.end(ctx);
}

// the bookkeeping kernel and the sums behind it; the totals' copy to the host is queued (rp_totals reads it after a
// synchronise: totals[2] = sum E on entry, on exit; counts[4] = E raised, E lowered, T raised, T lowered)
static int rp_book_run(sphx_ctx* ctx, bool cool, RpBook a, double* part, double* tot, StageTimer* t) {
    hipStream_t st = ctx->stream;
    const dim3 grid(sphx_blocks((size_t)a.n, RP_WG));
    if (cool) hipLaunchKernelGGL(rp_book_kernel<true>, grid, dim3(RP_WG), rp_lds_bytes(a.s, 3), st, a);
    else hipLaunchKernelGGL(rp_book_kernel<false>, grid, dim3(RP_WG), rp_lds_bytes(a.s, 3), st, a);
    HIPCHK(hipGetLastError());
    if (t) SPHX_TRY(t->mark(ctx, 2));
    SPHX_TRY(sphx_ordered_totals(ctx, a.n, RQ_N, a.pp, part, tot));
    return t ? t->mark(ctx, 3) : SPHX_OK;
}
static void rp_totals(sphx_ctx* ctx, double* totals, int64_t* counts) {
    double t[RQ_N];
    std::memcpy(t, ctx->pinned->scal, sizeof(t));
    if (totals) { totals[0] = t[RQ_EIN]; totals[1] = t[RQ_EOUT]; }
    if (counts) for (int q = 0; q < 4; ++q) counts[q] = (int64_t)t[RQ_ELO + q];
}
static int rp_check_const(sphx_ctx* ctx, const char* who, const SphxRpConst& c, bool cool) {
    if (!sphx_finite(c.t_cmb) || !sphx_finite(c.t_max) || !sphx_finite(c.k) || !sphx_finite(c.m_h))
        return sphx_set_err(ctx, SPHX_E_ARG, "%s: t_cmb, t_max, k_B and m_h must be finite", who);
    if (cool && (!sphx_finite(c.sb) || !sphx_finite(c.dt) || !sphx_finite(c.cooling_timescale) || c.cooling_timescale == 0.0))
        return sphx_set_err(ctx, SPHX_E_ARG, "%s: sb, dt and cooling_timescale must be finite, cooling_timescale not 0", who);
    return SPHX_OK;
}

// the two bookkeeping array calls: one body, the cooling's extra arrays NULL for the heating
static int rp_book_host(sphx_ctx* ctx, const char* who, bool cool, int64_t n, int s, int64_t n_gas, const double* f_un, const double* ptypes,
                        const double* mass, const double* E, const double* T, const double* mu_before, const double* sizes,
                        const double* energy, const double* vel, const double* lf2, const double* mom, const double* mu_specie,
                        const double* gamma_specie, const double* cross_sections, const SphxRpConst& c, double* mu_out, double* gam_out,
                        double* cross_out, double* E_out, double* T_out, double* vel_out, double* totals, int64_t* counts) {
    SPHX_TRY(rp_check(ctx, who, n, s, n_gas));
    SPHX_TRY(rp_check_const(ctx, who, c, cool));
    HIPCHK(hipSetDevice(ctx->device));
    SPHX_TRY(ctx->radphase_t.begin(ctx));
    const size_t nn = (size_t)n, ns = nn * (size_t)s, ng = (size_t)n_gas, nchunk = sphx_tot_chunks(n);
    double *d_f, *d_pt, *d_m, *d_E, *d_T, *d_x, *d_en, *d_mu, *d_g, *d_cr, *d_Eo, *d_To, *d_v, *d_vo, *d_lf2, *d_mom, *d_tab, *d_pp, *d_part, *d_tot;
    Carve b;
    b.take(d_f, ns, RP_AL);
    for (double** v : {&d_pt, &d_m, &d_E, &d_T, &d_x, &d_en, &d_mu, &d_g, &d_cr, &d_Eo, &d_To}) b.take(*v, nn, RP_AL);
    b.take(d_v, 3 * nn, RP_AL); b.take(d_vo, 3 * nn, RP_AL); b.take(d_lf2, ng, RP_AL); b.take(d_mom, 3 * ng, RP_AL);
    b.take(d_tab, 3 * (size_t)s, RP_AL); b.take(d_pp, RQ_N * nn, RP_AL); b.take(d_part, RQ_N * nchunk, RP_AL); b.take(d_tot, RQ_N, RP_AL);
    b.slack(8 * sizeof(double));
    SPHX_TRY(sphx_carve_into(ctx, ctx->radphase_buf, b));
    double* tab = ctx->radphase_tab;
    std::memcpy(tab, mu_specie, (size_t)s * sizeof(double));
    std::memcpy(tab + s, gamma_specie, (size_t)s * sizeof(double));
    std::memcpy(tab + 2 * s, cross_sections, (size_t)s * sizeof(double));
    // d_x: mu_before (heat) or sizes (cool)
    const CopyF64 us[] = {{f_un, d_f, ns}, {ptypes, d_pt, nn}, {mass, d_m, nn}, {E, d_E, nn}, {T, d_T, nn}, {cool ? sizes : mu_before, d_x, nn},
                          {cool ? energy : nullptr, d_en, nn}, {cool ? vel : nullptr, d_v, 3 * nn}, {n_gas > 0 ? lf2 : nullptr, d_lf2, ng},
                          {cool && n_gas > 0 ? mom : nullptr, d_mom, 3 * ng}, {tab, d_tab, 3 * (size_t)s}};
    SPHX_TRY(sphx_upload_f64(ctx, us, 11));
    int* off;
    SPHX_TRY(rp_ordinals(ctx, who, n, d_pt, n_gas, &off));
    RpBook a;
    a.n = (int)n; a.s = s;
    a.f = d_f; a.pt = d_pt; a.m = d_m; a.E = d_E; a.T = d_T;
    a.mu_before = cool ? nullptr : d_x; a.sizes = cool ? d_x : nullptr; a.energy = d_en; a.vel = d_v; a.mom = d_mom; a.lf2 = d_lf2;
    a.off = off; a.tab = d_tab; a.c = c;
    a.mu_out = d_mu; a.gam_out = d_g; a.cross_out = d_cr; a.E_out = d_Eo; a.T_out = d_To; a.vel_out = d_vo; a.pp = d_pp;
    SPHX_TRY(ctx->radphase_t.mark(ctx, 1));
    SPHX_TRY(rp_book_run(ctx, cool, a, d_part, d_tot, &ctx->radphase_t));
    const CopyF64 ds[] = {{mu_out, d_mu, nn}, {gam_out, d_g, nn}, {cross_out, d_cr, nn}, {E_out, d_Eo, nn}, {T_out, d_To, nn},
                          {cool ? vel_out : nullptr, d_vo, 3 * nn}};
    SPHX_TRY(sphx_download_f64(ctx, ds, 6));
    SPHX_TRY(ctx->radphase_t.mark(ctx, 4));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    rp_totals(ctx, totals, counts);
    return ctx->radphase_t.end(ctx);
}

extern "C" int sphx_rad_heat_bookkeeping(sphx_ctx* ctx, int64_t n, int s, int64_t n_gas, const double* f_un, const double* ptypes,
                                         const double* mass, const double* mu_before, const double* E_internal, const double* T,
                                         const double* lf2, const double* mu_specie, const double* gamma_specie,
                                         const double* cross_sections, double t_cmb, double t_max, double k_B, double m_h,
                                         double* mu_out, double* gamma_out, double* cross_out, double* E_out, double* T_out,
                                         double* totals, int64_t* counts) {
    if (!ctx) return SPHX_E_ARG;
    NEED(f_un); NEED(ptypes); NEED(mass); NEED(mu_before); NEED(E_internal); NEED(T); NEED(mu_specie); NEED(gamma_specie);
    NEED(cross_sections); NEED(mu_out); NEED(gamma_out); NEED(cross_out); NEED(E_out); NEED(T_out);
    if (n_gas > 0) NEED(lf2);
    SphxRpConst c;
    c.t_cmb = t_cmb; c.t_max = t_max; c.k = k_B; c.m_h = m_h; c.sb = 0.0; c.cooling_timescale = 1.0; c.dt = 0.0;
    return rp_book_host(ctx, "sphx_rad_heat_bookkeeping", false, n, s, n_gas, f_un, ptypes, mass, E_internal, T, mu_before, nullptr, nullptr,
                        nullptr, lf2, nullptr, mu_specie, gamma_specie, cross_sections, c, mu_out, gamma_out, cross_out, E_out, T_out,
                        nullptr, totals, counts);
}

extern "C" int sphx_rad_cool_bookkeeping(sphx_ctx* ctx, int64_t n, int s, int64_t n_gas, const double* final_comp, const double* energy,
                                         const double* ptypes, const double* mass, const double* sizes, const double* E_internal,
                                         const double* T, const double* velocities, const double* lf2, const double* momentum,
                                         const double* mu_specie, const double* gamma_specie, const double* cross_sections, double dt,
                                         double t_cmb, double t_max, double cooling_timescale, double sb, double k_B, double m_h,
                                         double* mu_out, double* gamma_out, double* cross_out, double* E_out, double* T_out,
                                         double* vel_out, double* totals, int64_t* counts) {
    if (!ctx) return SPHX_E_ARG;
    NEED(final_comp); NEED(energy); NEED(ptypes); NEED(mass); NEED(sizes); NEED(E_internal); NEED(T); NEED(velocities);
    NEED(mu_specie); NEED(gamma_specie); NEED(cross_sections); NEED(mu_out); NEED(gamma_out); NEED(cross_out); NEED(E_out);
    NEED(T_out); NEED(vel_out);
    if (n_gas > 0) { NEED(lf2); NEED(momentum); }
    SphxRpConst c;
    c.t_cmb = t_cmb; c.t_max = t_max; c.k = k_B; c.m_h = m_h; c.sb = sb; c.cooling_timescale = cooling_timescale; c.dt = dt;
    return rp_book_host(ctx, "sphx_rad_cool_bookkeeping", true, n, s, n_gas, final_comp, ptypes, mass, E_internal, T, nullptr, sizes, energy,
                        velocities, lf2, momentum, mu_specie, gamma_specie, cross_sections, c, mu_out, gamma_out, cross_out, E_out, T_out,
                        vel_out, totals, counts);
}

// =====================================================================================================================
// the whole block on the resident state: sphx_state_rad_phase
// =====================================================================================================================
// The state goes into the caller's particle order (the order of upload; sphx_phase_gather, sphx_phase.hip), in which every
// stage then runs: the bits are those of the array calls on the downloaded state.  The new velocities, E, T, mu, gamma
// (and drag coefficients) go back into the storage slots by sphx_phase_back.
// cross_array of drv:434 from dense rows: sum_t f cross_sections / sum_t f, t = 0 .. s - 1 (compat.cross_array_of's order)
__global__ __launch_bounds__(256) void rs_cross_kernel(int n, int s, const double* __restrict__ f, const double* __restrict__ tab, double* cross) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double mu, gamma, cr;
    sphx_rp_tables(s, f + (size_t)i * s, tab, tab + s, tab + 2 * s, &mu, &gamma, &cr);
    cross[i] = cr;
}
// the positions of the particles ids[q] (caller ids), q < count, from the gathered (n,3) positions
__global__ __launch_bounds__(256) void rs_pick_kernel(int count, const int* __restrict__ ids, const double* __restrict__ pos, double* out) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= count) return;
    const size_t i = (size_t)ids[q];
    out[3 * (size_t)q] = pos[3 * i]; out[3 * (size_t)q + 1] = pos[3 * i + 1]; out[3 * (size_t)q + 2] = pos[3 * i + 2];
}

extern "C" int sphx_state_rad_phase(sphx_ctx* ctx, double dt, double d, int64_t n_src, const int64_t* source_ids, const double* luminosities,
                                    int64_t n_dst, const int64_t* target_ids, const double* frac_dest, double photons_per_joule,
                                    const double* mu_specie, const double* gamma_specie, const double* cross_sections,
                                    const double* driver_cross_sections, double amu, double t_cmb, double t_max,
                                    double cooling_timescale, double sb, double k_B, double m_h, int mode, const double* grain_mass,
                                    const double* sigma_effective, double* cross_array, double* lf2, double* momentum,
                                    double* extinction, double* f_un_ionised, double* frac_destroyed, double* heat_out /* (5,n) */,
                                    double* energy, double* rec_array, double* cross_out, double* totals /* [3] */,
                                    int64_t* counts /* int64[8] */, int64_t* n_gas_out, int* skipped) {
    if (!ctx) return SPHX_E_ARG;
    const char* who = "sphx_state_rad_phase";
    SPHX_TRY(sphx_phase_need_list(ctx, who));
    if (ctx->s < 6 || !ctx->fun_id.p)
        return sphx_set_err(ctx, SPHX_E_STATE, "%s: the state carries no composition (f_un) of >= 6 species", who);
    const int64_t n = ctx->n;
    const int k = ctx->k, s = ctx->s, sp = ctx->sp;
    NEED(frac_dest); NEED(mu_specie); NEED(gamma_specie); NEED(cross_sections); NEED(driver_cross_sections); NEED(skipped);
    SPHX_TRY(rp_check(ctx, who, n, s, 0));
    SPHX_TRY(sphx_cool_check(ctx, who, n, k, s, dt, d));
    SphxRpConst c;
    c.t_cmb = t_cmb; c.t_max = t_max; c.k = k_B; c.m_h = m_h; c.sb = sb; c.cooling_timescale = cooling_timescale; c.dt = dt;
    SPHX_TRY(rp_check_const(ctx, who, c, true));
    if (n_src < 0 || n_dst < 0 || n_src > (1ll << 24) || n_dst > (1ll << 24))
        return sphx_set_err(ctx, SPHX_E_ARG, "%s: n_src=%lld, n_dst=%lld out of range", who, (long long)n_src, (long long)n_dst);
    if (n_src > 0) { NEED(source_ids); NEED(luminosities); }
    if (n_dst > 0) NEED(target_ids);
    for (int64_t q = 0; q < n_src; ++q)
        if (source_ids[q] < 0 || source_ids[q] >= n) return sphx_set_err(ctx, SPHX_E_ARG, "%s: source id %lld outside [0, n)", who, (long long)source_ids[q]);
    for (int64_t q = 0; q < n_dst; ++q)
        if (target_ids[q] < 0 || target_ids[q] >= n) return sphx_set_err(ctx, SPHX_E_ARG, "%s: target id %lld outside [0, n)", who, (long long)target_ids[q]);
    SPHX_TRY(sphx_phase_check_tables(ctx, who, s, gamma_specie, grain_mass, sigma_effective));
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t stream = ctx->stream;
    const StateArrays& st = ctx->st;
    const size_t nn = (size_t)n, npad = (size_t)sphx_pad64(n), ns = nn * (size_t)s, ss = (size_t)s;
    *skipped = 0;
    // ---- drv:243: no star, no block.  The ordinals are those of the storage slots here, and only their number is used ----
    int* off_slots;
    int64_t ng = 0;
    SPHX_TRY(rp_ordinals(ctx, who, n, st.ptype.as<double>(), -1, &off_slots, &ng));
    if (n_gas_out) *n_gas_out = ng;
    if (ng == n) { *skipped = 1; return SPHX_OK; }
    SPHX_TRY(ctx->radstate_t.begin(ctx));
    // ---- buffers ----
    const size_t nchunk = sphx_tot_chunks(n), g = (size_t)ng;
    double *g_pos, *g_x, *g_y, *g_z, *g_vel, *g_m, *g_mu, *g_h, *g_T, *g_pt, *g_E, *f0, *f1, *cross0, *d_fr, *h_mu, *h_g, *h_cr, *h_E, *h_T;
    double *c_mu, *c_g, *c_cr, *c_E, *c_T, *c_vel, *d_mgm, *d_mcs, *d_src, *d_dst, *d_tab, *d_pp, *d_part, *d_tot;
    CarveN<40> b;
    b.take(g_pos, 3 * nn, RP_AL); b.take(g_x, nn, RP_AL); b.take(g_y, nn, RP_AL); b.take(g_z, nn, RP_AL); b.take(g_vel, 3 * nn, RP_AL);
    for (double** v : {&g_m, &g_mu, &g_h, &g_T, &g_pt, &g_E}) b.take(*v, nn, RP_AL);
    b.take(f0, ns, RP_AL); b.take(f1, ns, RP_AL); b.take(cross0, nn, RP_AL); b.take(d_fr, 3 * g, RP_AL);
    for (double** v : {&h_mu, &h_g, &h_cr, &h_E, &h_T, &c_mu, &c_g, &c_cr, &c_E, &c_T}) b.take(*v, nn, RP_AL);
    b.take(c_vel, 3 * nn, RP_AL); b.take(d_mgm, nn, RP_AL); b.take(d_mcs, nn, RP_AL);
    b.take(d_src, 3 * (size_t)n_src, RP_AL); b.take(d_dst, 3 * (size_t)n_dst, RP_AL);
    b.take(d_tab, 8 * ss, RP_AL); b.take(d_pp, RQ_N * nn, RP_AL); b.take(d_part, RQ_N * nchunk, RP_AL); b.take(d_tot, RQ_N, RP_AL);
    b.slack(16 * sizeof(double));
    SPHX_TRY(sphx_carve_into(ctx, ctx->radstate_buf, b));
    int *col, *list, *d_ids;                         // ids: the sources', then the targets', and one more
    Carve bi;
    bi.take(col, npad); bi.take(list, (size_t)k * npad); bi.take(d_ids, (size_t)(n_src + n_dst) + 1);
    bi.pad(16);
    SPHX_TRY(sphx_carve_into(ctx, ctx->radstate_int, bi));
    // tables: [0,3s) mu_specie | nsc cross_sections | frac_dest (ionise); [3s,6s) mu_specie | gamma | driver cross (bookkeeping);
    // [6s,8s) grain_mass | sigma_effective
    double* tab = ctx->radstate_tab;                 // (held by the context: the upload below reads it)
    for (int t = 0; t < s; ++t) {
        tab[t] = mu_specie[t]; tab[s + t] = cross_sections[t]; tab[2 * s + t] = frac_dest[t];
        tab[3 * s + t] = mu_specie[t]; tab[4 * s + t] = gamma_specie[t]; tab[5 * s + t] = driver_cross_sections[t];
        tab[6 * s + t] = ctx->drag ? grain_mass[t] : 0.0; tab[7 * s + t] = ctx->drag ? sigma_effective[t] : 0.0;
    }
    HIPCHK(hipMemcpyAsync(d_tab, tab, 8 * ss * sizeof(double), hipMemcpyHostToDevice, stream));
    std::vector<int> ids((size_t)(n_src + n_dst));
    for (int64_t q = 0; q < n_src; ++q) ids[(size_t)q] = (int)source_ids[q];
    for (int64_t q = 0; q < n_dst; ++q) ids[(size_t)(n_src + q)] = (int)target_ids[q];
    if (!ids.empty()) HIPCHK(hipMemcpy(d_ids, ids.data(), ids.size() * sizeof(int), hipMemcpyHostToDevice));   // (pageable, so synchronous)
    // ---- 1, 2: the state through st.id; the list into caller ids; the dense rows; cross_array; the rays' ends ----
    PhaseGather ga;
    ga.n = (int)n; ga.qorder = ctx->step_qorder; ga.id = st.id.as<int>();
    ga.x = st.x.as<double>(); ga.y = st.y.as<double>(); ga.z = st.z.as<double>();
    ga.vx = st.vx.as<double>(); ga.vy = st.vy.as<double>(); ga.vz = st.vz.as<double>();
    ga.m = st.m.as<double>(); ga.mu = st.mu.as<double>(); ga.h = sphx_phase_sizes(ctx); ga.T = st.T.as<double>();
    ga.pt = st.ptype.as<double>(); ga.E = st.E.as<double>();
    ga.col = col; ga.pos = g_pos; ga.sx = g_x; ga.sy = g_y; ga.sz = g_z; ga.vel = g_vel; ga.om = g_m; ga.omu = g_mu; ga.oh = g_h;
    ga.oT = g_T; ga.opt = g_pt; ga.oE = g_E;
    SPHX_TRY(sphx_phase_gather(ctx, ga));
    SPHX_TRY(sphx_phase_translate(ctx, col, true, list));
    HIPCHK(hipMemcpy2DAsync(f0, ss * sizeof(double), ctx->fun_id.p, (size_t)sp * sizeof(double), ss * sizeof(double), nn,
                            hipMemcpyDeviceToDevice, stream));
    hipLaunchKernelGGL(rs_cross_kernel, dim3(sphx_blocks(nn, 256)), dim3(256), 0, stream, (int)n, s, f0, d_tab + 3 * ss, cross0);
    if (n_src > 0) hipLaunchKernelGGL(rs_pick_kernel, dim3(sphx_blocks((size_t)n_src, 256)), dim3(256), 0, stream, (int)n_src, d_ids, g_pos, d_src);
    if (n_dst > 0) hipLaunchKernelGGL(rs_pick_kernel, dim3(sphx_blocks((size_t)n_dst, 256)), dim3(256), 0, stream, (int)n_dst, d_ids + n_src, g_pos, d_dst);
    HIPCHK(hipGetLastError());
    SPHX_TRY(ctx->radstate_t.mark(ctx, 1));
    // ---- 3: nsc:922-965 ----
    RadDevOut rad;
    SPHX_TRY(sphx_rad_run_dev(ctx, who, n, g_x, g_y, g_z, g_m, g_pt, g_h, cross0, g_mu, n_src, d_src, luminosities, n_dst, d_dst, dt, mode, &rad));
    if (rad.ng != ng) return sphx_set_err(ctx, SPHX_E_HIP, "%s: %lld non-star particles, the transfer met %lld", who, (long long)ng, (long long)rad.ng);
    SPHX_TRY(ctx->radstate_t.mark(ctx, 2));
    // ---- 4, 5: nsc:976-1012, drv:258-273 (the ordinals now in caller order) ----
    int* off;
    SPHX_TRY(rp_ordinals(ctx, who, n, g_pt, ng, &off));
    RpIon ia;
    ia.n = (int)n; ia.s = s;
    ia.f_in = f0; ia.m = g_m; ia.pt = g_pt; ia.lf2 = rad.lf2; ia.off = off; ia.tab = d_tab;
    ia.ppj = photons_per_joule; ia.amu = amu;
    ia.f_out = f1; ia.frac = frac_destroyed ? d_fr : nullptr;
    hipLaunchKernelGGL(rp_ionise_kernel, dim3(sphx_blocks(nn, RP_WG)), dim3(RP_WG), rp_lds_bytes(s, 3), stream, ia);
    HIPCHK(hipGetLastError());
    RpBook ha;
    ha.n = (int)n; ha.s = s;
    ha.f = f1; ha.pt = g_pt; ha.m = g_m; ha.E = g_E; ha.T = g_T;
    ha.mu_before = g_mu; ha.sizes = nullptr; ha.energy = nullptr; ha.vel = nullptr; ha.mom = nullptr; ha.lf2 = rad.lf2;
    ha.off = off; ha.tab = d_tab + 3 * ss; ha.c = c;
    ha.mu_out = h_mu; ha.gam_out = h_g; ha.cross_out = h_cr; ha.E_out = h_E; ha.T_out = h_T; ha.vel_out = nullptr; ha.pp = d_pp;
    SPHX_TRY(rp_book_run(ctx, false, ha, d_part, d_tot, nullptr));
    SPHX_TRY(ctx->radstate_t.mark(ctx, 3));
    HIPCHK(hipStreamSynchronize(stream));                                    // (the totals leave the pinned block before the cooling's count lands in it)
    double tot_heat[2];
    int64_t cnt_heat[4];
    rp_totals(ctx, tot_heat, cnt_heat);
    // ---- 6: nsc:1019-1176 on the step's list; sizes is never read there, h(m) comes from d ----
    const CoolDev cin{g_pos, g_pt, g_m, h_mu, h_T, f1};
    CoolRes cres;
    SPHX_TRY(sphx_cool_run(ctx, who, n, k, s, cin, nullptr, list, dt, d, nullptr, &cres));
    SPHX_TRY(ctx->radstate_t.mark(ctx, 4));
    // ---- 7: drv:283-311 ----
    RpBook ca = ha;
    ca.f = cres.final_comp; ca.E = h_E; ca.T = h_T;
    ca.mu_before = nullptr; ca.sizes = g_h; ca.energy = cres.energy; ca.vel = g_vel; ca.mom = rad.mom;
    ca.mu_out = c_mu; ca.gam_out = c_g; ca.cross_out = c_cr; ca.E_out = c_E; ca.T_out = c_T; ca.vel_out = c_vel;
    SPHX_TRY(rp_book_run(ctx, true, ca, d_part, d_tot, nullptr));
    // ---- 8: the write-back through st.id; the composition rows into fun_id ----
    if (ctx->drag) SPHX_TRY(sphx_phase_drag_refresh(ctx, n, s, cres.final_comp, d_tab + 6 * ss, d_tab + 7 * ss, d_mgm, d_mcs));
    const PhaseBack ba{(int)n, st.id.as<int>(), c_vel, st.vx.as<double>(), st.vy.as<double>(), st.vz.as<double>(), ctx->drag ? 6 : 4,
                       {c_E, c_T, c_mu, c_g, d_mgm, d_mcs},
                       {st.E.as<double>(), st.T.as<double>(), st.mu.as<double>(), st.gam.as<double>(), st.mgm.as<double>(), st.mcs.as<double>()}};
    SPHX_TRY(sphx_phase_back(ctx, ba));
    HIPCHK(hipMemcpy2DAsync(ctx->fun_id.p, (size_t)sp * sizeof(double), cres.final_comp, ss * sizeof(double), ss * sizeof(double), nn,
                            hipMemcpyDeviceToDevice, stream));
    const CopyF64 ds[] = {{cross_array, cross0, nn}, {lf2, rad.lf2, g}, {momentum, rad.mom, 3 * g}, {extinction, rad.ext, g},
                          {f_un_ionised, f1, ns}, {frac_destroyed, d_fr, 3 * g}, {heat_out, h_mu, nn},
                          {heat_out ? heat_out + nn : nullptr, h_g, nn}, {heat_out ? heat_out + 2 * nn : nullptr, h_cr, nn},
                          {heat_out ? heat_out + 3 * nn : nullptr, h_E, nn}, {heat_out ? heat_out + 4 * nn : nullptr, h_T, nn},
                          {energy, cres.energy, nn}, {rec_array, cres.rec_array, ns}, {cross_out, c_cr, nn}};
    SPHX_TRY(sphx_download_f64(ctx, ds, 14));
    SPHX_TRY(ctx->radstate_t.mark(ctx, 5));
    HIPCHK(hipStreamSynchronize(stream));
    double tot_cool[2];
    int64_t cnt_cool[4];
    rp_totals(ctx, tot_cool, cnt_cool);
    if (totals) { totals[0] = tot_heat[0]; totals[1] = tot_heat[1]; totals[2] = tot_cool[1]; }
    if (counts) for (int q = 0; q < 4; ++q) { counts[q] = cnt_heat[q]; counts[4 + q] = cnt_cool[q]; }
    return ctx->radstate_t.end(ctx);
}
